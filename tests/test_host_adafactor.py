"""Host side of the fused Adafactor optimizer (no GPU): the float64 reference against the HF class, adafactor_layout on the SDXL shape
table, config keys and errors, optimizer_type selection in the full, the LoRA and the drop-in trainer, the state round trip, the struct
mirrors, the C-ABI argument errors of algorithm 3, and the bounds of tests/_adafactor_ref.py tried on single defects."""
import ctypes as C
import importlib
import logging
import math
import re
import shutil
import subprocess
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import _adafactor_ref as R
import sdxl_amd  # noqa: F401
from oracle import unet_ref as U
from sdxl_amd import lib
from _optim_common import StandInNet

T = importlib.import_module("sdxl-training-improvements_amd.trainer")
O = importlib.import_module("sdxl-training-improvements_amd.optimizer")
NM = importlib.import_module("sdxl-training-improvements_amd.native_mi355x")
CFG = importlib.import_module("sdxl-training-improvements_amd.config")
LORA = importlib.import_module("sdxl-training-improvements_amd.lora")
ROOT = Path(__file__).resolve().parent.parent

RECIPES = {"defaults": dict(), "sdxl_full_finetune": dict(lr=4e-7, scale_parameter=False, relative_step=False)}


# ---------------------------------------------------------------------------------------------- the reference against the HF class
@pytest.mark.parametrize("recipe", list(RECIPES))
@pytest.mark.parametrize("extra", [dict(), dict(beta1=0.9), dict(weight_decay=0.1), dict(beta1=0.9, weight_decay=0.1)], ids=["plain", "beta1", "wd", "beta1_wd"])
def test_reference_equals_the_hf_class(recipe, extra):
    """5 steps of transformers.optimization.Adafactor on CPU float32 tensors against step64 carried in float64.  4-D tensors are handed to
    the HF class as [out][rest] (this project's factoring).  The bound per step is the float32 rounding of HF's own arithmetic: its row
    and column means add cols and rows terms (at most (N - 1) 2^-24 relative each, both enter the update through square roots, and the
    mean of R' adds rows more), its RMS sums stay below 64 * 2^-24 relative (torch's blocked sums), and about a dozen single operations;
    so the update differs by at most (rows + cols + 64) 2^-24 of its size, and the parameter by 2^-23 of its own per step on top."""
    hf = pytest.importorskip("transformers").optimization.Adafactor
    kw = {**RECIPES[recipe], **extra}
    hp = R.Hyper(**kw)
    g0 = torch.Generator().manual_seed(3)
    shapes = [(37, 72), (16, 8, 3, 3), (320,), (4, 2880)]
    params = [torch.nn.Parameter(torch.randn(s[0], int(np.prod(s[1:])), generator=g0) * 0.05 if len(s) > 1 else torch.randn(*s, generator=g0) * 0.05)
              for s in shapes]
    opt = hf(params, lr=kw.get("lr"), eps=hp.eps, clip_threshold=hp.clip_threshold, decay_rate=hp.decay_rate, beta1=hp.beta1,
             weight_decay=hp.weight_decay, scale_parameter=hp.scale_parameter, relative_step=hp.relative_step, warmup_init=hp.warmup_init)
    ents, xs, states, ms = [], [], [], []
    for p in params:
        rows, cols = (p.shape[0], p.shape[1]) if p.dim() == 2 else (1, p.shape[0])
        e = R.Entry(0, rows, cols, rows * cols, p.dim() == 2, 0)
        ents.append(e)
        xs.append(p.detach().double().numpy().reshape(rows, cols).copy())
        states.append({"R": np.zeros(rows), "C": np.zeros(cols)} if e.factored else {"v": np.zeros((rows, cols))})
        ms.append(np.zeros((rows, cols)))
    worst = 0.0
    for k in range(1, 6):
        # the scalars in full double precision here: the HF class does not round them to float32 first
        sc = R.Scalars(hp.beta2t(k), 1.0 - hp.beta2t(k), hp.rho(k), hp.eps[0], hp.eps[1], hp.clip_threshold, hp.beta1 or 0.0,
                       1.0 - (hp.beta1 or 0.0), hp.weight_decay, hp.scale_parameter, hp.beta1 is not None)
        grads = [torch.randn(p.shape, generator=g0) * (0.5 if i % 2 else 3.0) for i, p in enumerate(params)]
        for p, g in zip(params, grads):
            p.grad = g.clone()
        opt.step()
        for i, (e, p, g) in enumerate(zip(ents, params, grads)):
            ref = R.step64(e, g.double().numpy().reshape(e.rows, e.cols), xs[i], states[i], ms[i], sc)
            xs[i], ms[i] = ref["x"], ref["m"] if ref["m"] is not None else ms[i]
            states[i] = {"R": ref["R"], "C": ref["C"]} if e.factored else {"v": ref["v"]}
            got = p.detach().double().numpy().reshape(e.rows, e.cols)
            step_size = np.abs(ref["d"]) + np.abs(ref["dx"])
            bound = k * ((e.rows + e.cols + 64) * R.U * float(step_size.max()) + 2 * R.U * float(np.abs(got).max()))
            diff = float(np.abs(got - ref["x"]).max())
            worst = max(worst, diff / bound)
            assert diff <= bound, (recipe, extra, k, shapes[i], diff, bound)
            assert float(np.abs(ref["d"]).max()) > 0
    print(f"[{recipe} {extra}] largest used fraction of the bound over 5 steps: {worst:.3f}")


# ---------------------------------------------------------------------------------------------- the layout
def sdxl_table():
    """the SDXL UNet's state-dict shapes with arena ranges as the engine lays them out: every tensor on a 64-element boundary, a 3 x 3
    convolution as [cout][9][cin padded to 8]"""
    shapes = {k: tuple(int(x) for x in v) for k, v in U.param_shapes().items()}
    ranges, cur = {}, 0
    for k, s in shapes.items():
        n = int(np.prod(s))
        if len(s) == 4 and s[2] == 3:
            n = s[0] * 9 * ((s[1] + 7) // 8 * 8)
        ranges[k] = (cur, n)
        cur = (cur + n + 63) // 64 * 64
    return shapes, ranges, cur


def test_layout_of_the_sdxl_shape_table():
    shapes, ranges, total = sdxl_table()
    ents = O.adafactor_layout(shapes, ranges)
    assert sorted(e.name for e in ents) == sorted(shapes) and len({e.name for e in ents}) == len(shapes)        # every tensor once
    assert all(a.elem_off + a.rows * a.cols <= b.elem_off for a, b in zip(ents, ents[1:]))                      # sorted, no overlap
    assert ents[-1].elem_off + ents[-1].rows * ents[-1].cols <= total
    by = {e.name: e for e in ents}
    for e in ents:
        s = shapes[e.name]
        assert e.elem_off == ranges[e.name][0] and e.elem_off % 8 == 0 and e.cols % 8 == 0 and e.numel == int(np.prod(s))
        if len(s) == 1:
            assert not e.factored and e.rows == 1 and e.cols == (s[0] + 7) // 8 * 8
        elif e.name != "conv_in.weight":
            assert e.factored and (e.rows, e.cols) == (s[0], int(np.prod(s[1:]))) and e.numel == e.rows * e.cols, e
    ci = by["conv_in.weight"]
    assert not ci.factored and (ci.rows, ci.cols, ci.numel) == (320, 72, 320 * 4 * 9)          # pad channels inside its range
    co = by["conv_out.weight"]
    assert co.factored and (co.rows, co.cols) == (4, 2880)
    ff = next(e for e in ents if e.name.endswith("ff.net.0.proj.weight") and shapes[e.name] == (10240, 1280))
    assert ff.factored and (ff.rows, ff.cols) == (10240, 1280)                                 # a plain matrix: its row order is R's
    state = sum(e.state_floats() for e in ents)
    params = sum(e.numel for e in ents)
    scratch = O.adafactor_scratch_floats(ents)
    assert scratch == R.scratch_floats([R.Entry(e.elem_off, e.rows, e.cols, e.numel, e.factored, 0) for e in ents])
    print(f"SDXL UNet: {len(ents)} tensors, {params} parameters, {sum(e.factored for e in ents)} factored; Adafactor statistics {state} floats "
          f"({4 * state / params:.4f} B per parameter against AdamW_BF16's 4 B of moments), scratch {scratch} floats")
    assert params > 2.5e9 and state < params // 300
    with pytest.raises(ValueError, match="overlaps"):
        O.adafactor_layout({"a": (8,), "b": (8,)}, {"a": (0, 8), "b": (0, 8)})
    with pytest.raises(ValueError, match="multiple of 8"):
        O.adafactor_layout({"a": (8,)}, {"a": (4, 8)})


def test_layout_of_an_adapter_arena_and_refusal_of_other_algorithms():
    from test_host_lora import StandInNet as TinyTable
    net = TinyTable()
    ad = LORA.LoRAAdapters(net, rank=4)
    o = O.AdafactorBF16(ad, lr=1e-3)
    assert len(o.entries) == 2 * len(ad.targets)
    pr = ad.param_ranges()
    for e in o.entries:
        assert e.elem_off == pr[e.name][0]
        if e.name.endswith("lora_A.weight"):
            assert e.factored and e.rows == 4 and e.numel == e.rows * e.cols
        else:                                             # [out][4]: rows shorter than a 16-byte vector run unfactored
            assert not e.factored and e.rows == 1 and e.cols == pr[e.name][1] and e.numel % 4 == 0
    ad8 = LORA.LoRAAdapters(net, rank=8)
    assert all(e.factored for e in O.AdafactorBF16(ad8, lr=1e-3).entries)
    for algo in ("loha", "kronecker", "dora"):
        with pytest.raises(ValueError, match=algo):
            O.AdafactorBF16(LORA.LoRAAdapters(net, rank=4, algo=algo, kinds="all"), lr=1e-3)


# ---------------------------------------------------------------------------------------------- config, trainers
def test_yaml_keys_defaults_and_errors(tmp_path):
    d = CFG.Config().optimizer
    assert (tuple(d.eps), d.clip_threshold, d.decay_rate, d.adafactor_beta1, d.scale_parameter, d.relative_step, d.warmup_init) == \
        ((1e-30, 1e-3), 1.0, -0.8, None, True, True, False)
    p = tmp_path / "c.yaml"
    p.write_text("optimizer:\n  optimizer_type: adafactor\n  learning_rate: 4.0e-7\n  weight_decay: 0.0\n  scale_parameter: false\n"
                 "  relative_step: false\n  eps: [1.0e-30, 1.0e-3]\n  clip_threshold: 1.5\n  decay_rate: -0.7\n  adafactor_beta1: 0.9\n")
    cfg = CFG.Config.from_yaml(p)
    o = T.NativeSDXLTrainer(StandInNet(), device="cpu", config=cfg).optimizer
    assert type(o) is O.AdafactorBF16 and O.BY_TYPE["adafactor"] is O.AdafactorBF16 and O.AdafactorBF16.ZERO1 is False
    g = o.param_groups[0]
    assert (g["lr"], g["eps"], g["clip_threshold"], g["decay_rate"], g["beta1"], g["weight_decay"], g["scale_parameter"], g["relative_step"],
            g["warmup_init"]) == (4e-7, (1e-30, 1e-3), 1.5, -0.7, 0.9, 0.0, False, False, False)
    assert o.exp_avg.dtype == torch.float32 and o.exp_avg.untyped_storage().nbytes() == 4 * 64
    # the defaults: relative steps, no first moment, no arena-sized moments at all
    cfg = CFG.Config()
    cfg.optimizer.optimizer_type = "Adafactor"
    o = T.NativeSDXLTrainer(StandInNet(), device="cpu", config=cfg).optimizer
    assert type(o) is O.AdafactorBF16 and o.param_groups[0]["relative_step"] and o.param_groups[0]["lr"] is None
    assert o.exp_avg.numel() == o.exp_avg_sq.numel() == 64 and o.exp_avg.untyped_storage().nbytes() == o.exp_avg_sq.untyped_storage().nbytes() == 4
    assert o.comp.dtype == torch.bfloat16 and o.comp.numel() == 64 and o.moment_arenas() == (None, None)
    assert o.schedule() == (0.0, 1e-2)
    o.step_count = 3
    assert o.schedule() == (1.0 - math.pow(4, -0.8), 1e-2)
    o.step_count = 10 ** 6
    assert o.schedule()[1] == 1.0 / math.sqrt(10 ** 6 + 1)
    w = O.AdafactorBF16(StandInNet(), warmup_init=True)
    w.step_count = 4
    assert w.schedule()[1] == 1e-6 * 5
    with pytest.raises(lib.SdxlError):                   # no library behind the stand-in, no fallback
        o.step()
    # HF's errors
    cfg.optimizer.learning_rate = 4e-7                   # a manual lr together with relative_step
    with pytest.raises(ValueError, match="relative_step"):
        T.NativeSDXLTrainer(StandInNet(), device="cpu", config=cfg)
    with pytest.raises(ValueError, match="relative_step"):
        O.AdafactorBF16(StandInNet(), lr=1e-3, relative_step=True)
    with pytest.raises(ValueError, match="warmup_init"):
        O.AdafactorBF16(StandInNet(), lr=1e-3, relative_step=False, warmup_init=True)
    for kw in (dict(lr=-1.0), dict(eps=(1e-30,)), dict(eps=(-1.0, 1e-3)), dict(clip_threshold=0.0), dict(decay_rate=0.5), dict(beta1=1.0),
               dict(weight_decay=-0.1), dict(relative_step=False)):
        with pytest.raises(ValueError):
            O.AdafactorBF16(StandInNet(), **kw)
    # the other algorithms still allocate their two arena-sized moments
    for cls in (O.AdamWBF16, O.AdamWScheduleFreeKahanBF16, O.ProdigyBF16):
        a = cls(StandInNet())
        assert a.exp_avg.untyped_storage().nbytes() == a.exp_avg.element_size() * 64 == a.exp_avg_sq.untyped_storage().nbytes()
        assert a.moment_arenas() == (a.exp_avg, a.exp_avg_sq)


def test_shard_optimizer_rule_and_pieces():
    cfg = CFG.Config()
    cfg.optimizer.optimizer_type = "adafactor"
    cfg.training.shard_optimizer = True
    with pytest.raises(ValueError, match="training.shard_optimizer"):
        T.NativeSDXLTrainer(StandInNet(), device="cpu", config=cfg)
    cfg.training.shard_optimizer = None
    tr = T.NativeSDXLTrainer(StandInNet(), device="cpu", config=cfg)
    assert not tr.sharded and type(tr.sync).__name__ == "GradSync"
    with pytest.raises(ValueError, match="pieces"):
        O.AdafactorBF16(StandInNet(L=object())).step(torch.zeros(64), pieces=[(0, 8, 0)])


def test_lora_trainer_and_dropin_select_the_class(caplog):
    from test_host_lora import StandInNet as TinyTable
    cfg = CFG.Config()
    cfg.optimizer.optimizer_type, cfg.training.lora_rank = "adafactor", 4
    with caplog.at_level(logging.WARNING):
        tr = T.create_trainer(SimpleNamespace(unet=TinyTable()), config=cfg, device="cpu")
    assert isinstance(tr, LORA.NativeLoRATrainer) and type(tr.optimizer) is O.AdafactorBF16 and tr.optimizer.net is tr.lora and not caplog.records
    cfg.training.lora_algo = "loha"
    with pytest.raises(ValueError, match="loha"):
        T.create_trainer(SimpleNamespace(unet=TinyTable()), config=cfg, device="cpu")

    class Adafactor:                                     # stand-in with the HF class's name and its param_groups
        param_groups = [{"lr": 4e-7, "eps": (1e-30, 1e-3), "clip_threshold": 1.0, "decay_rate": -0.8, "beta1": None, "weight_decay": 0.0,
                         "scale_parameter": False, "relative_step": False, "warmup_init": False}]

    ref_cfg = SimpleNamespace(model=SimpleNamespace(model_type="sdxl"), optimizer=SimpleNamespace(optimizer_type="adamw_bf16"),
                              training=SimpleNamespace(method="native_mi355x"))
    one = NM.NativeMI355XTrainer(SimpleNamespace(unet=StandInNet()), optimizer=Adafactor(), device="cpu", config=ref_cfg)
    g = one.optimizer.param_groups[0]
    assert type(one.optimizer) is O.AdafactorBF16 and (g["lr"], g["scale_parameter"], g["relative_step"], g["beta1"], g["weight_decay"]) == \
        (4e-7, False, False, None, 0.0)
    ref_cfg.optimizer = SimpleNamespace(optimizer_type="adafactor", relative_step=False, scale_parameter=False, learning_rate=4e-7, weight_decay=0.0)
    two = NM.NativeMI355XTrainer(SimpleNamespace(unet=StandInNet()), device="cpu", config=ref_cfg)
    assert type(two.optimizer) is O.AdafactorBF16 and two.optimizer.param_groups[0]["lr"] == 4e-7


def test_state_dict_round_trip_and_refusals():
    a = O.AdafactorBF16(StandInNet(), lr=1e-3, beta1=0.9)
    a.af_state.copy_(torch.arange(a.af_state.numel(), dtype=torch.float32) + 1.0)
    a.comp.copy_(torch.arange(64, dtype=torch.float32) * 2 ** -12)
    a.exp_avg.copy_(torch.arange(64, dtype=torch.float32) * 0.5)
    a.step_count = 7
    sd = a.state_dict()
    assert sd["algorithm"] == "adafactor" and set(sd["state"]) == {"step", "af_state", "comp", "exp_avg"}
    b = O.AdafactorBF16(StandInNet(), lr=1e-3, beta1=0.9)
    b.load_state_dict(sd)
    assert b.step_count == 7 and torch.equal(a.af_state, b.af_state) and torch.equal(a.comp, b.comp) and torch.equal(a.exp_avg, b.exp_avg)
    assert len(b.state_arenas()) == 2 and set(O.AdafactorBF16(StandInNet()).state_dict()["state"]) == {"step", "af_state", "comp"}
    for other in (O.AdafactorBF16(StandInNet(), lr=1e-3), O.AdafactorBF16(StandInNet(), beta1=0.9), O.AdafactorBF16(StandInNet(), lr=1e-3, beta1=0.9, decay_rate=-0.7),
                  O.AdamWBF16(StandInNet()), O.ProdigyBF16(StandInNet())):
        with pytest.raises(ValueError):
            other.load_state_dict(sd)
    with pytest.raises(ValueError):
        b.load_state_dict(O.ProdigyBF16(StandInNet()).state_dict())
    E = importlib.import_module("sdxl-training-improvements_amd.ema")
    net = StandInNet()
    o = O.AdafactorBF16(net)
    ema = E.WeightEMA(net)
    o.attach_ema(ema)
    assert o.ema is ema


def test_table_lists_the_trainable_tensors_only():
    class Net(StandInNet):
        def __init__(self):
            super().__init__(n=192)
            self.live = None

        def param_shapes(self):
            return {"a.weight": (4, 16), "a.bias": (4,), "b.weight": (8, 8)}

        def param_ranges(self):
            return {"a.weight": (0, 64), "a.bias": (64, 4), "b.weight": (128, 64)}

        def trainable(self):
            return set(self.param_shapes()) if self.live is None else set(self.live)

    net = Net()
    o = O.AdafactorBF16(net)
    ents, arr = o.table()
    assert [e.name for e in ents] == ["a.weight", "a.bias", "b.weight"] and [e.factored for e in ents] == [True, False, True]
    assert [(arr[i].elem_off, arr[i].rows, arr[i].cols, arr[i].numel, arr[i].state_off) for i in range(3)] == \
        [(0, 4, 16, 64, 0), (64, 1, 8, 4, 20), (128, 8, 8, 64, 28)]
    assert o.af_state.numel() == 44 == o.state_floats()
    net.live = ["b.weight"]
    ents, arr = o.table()
    assert [e.name for e in ents] == ["b.weight"] and arr[0].state_off == 28            # the statistics keep their place


# ---------------------------------------------------------------------------------------------- the boundary
def test_struct_mirrors_and_the_boundary(tmp_path):
    text = (ROOT / "include" / "sdxlstep.h").read_text()
    names = lambda t: set(re.findall(r"\b(sdxl_[a-z0-9_]+)\s*\(", t))
    dh = (ROOT / "include" / "sdxlstep_diag.h").read_text()
    hooks = names(dh.split("part 2: experiment ABI", 1)[0].split("part 1: test hooks", 1)[1])
    assert len(names(text)) <= 58 and len(hooks) == 29
    assert f"#define SDXL_AF_ROWS {lib.AF_ROWS}" in text and f"#define SDXL_AF_COLS {lib.AF_COLS}" in text
    assert (lib.AF_ROWS, lib.AF_COLS) == (R.AF_ROWS, R.AF_COLS)
    cc = next((c for c in (shutil.which("cc"), shutil.which("gcc"), shutil.which("clang"), "/opt/rocm/lib/llvm/bin/clang") if c and Path(c).exists()), None)
    assert cc is not None, "no C compiler"
    tf = [n for n, _t in lib.AdafactorTensor._fields_]
    cf = ["clip_threshold", "eps1", "eps2", "beta2t", "rho", "scale_parameter", "use_beta1", "tensors", "n_tensors", "af_state", "af_scratch"]
    src = tmp_path / "offsets.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "sdxlstep.h"\nint main(void) {\n'
                   '  printf("%zu %zu\\n", sizeof(sdxl_adafactor_tensor), sizeof(sdxl_adamw_config));\n'
                   + "".join(f'  printf("%zu\\n", offsetof(sdxl_adafactor_tensor, {n}));\n' for n in tf)
                   + "".join(f'  printf("%zu\\n", offsetof(sdxl_adamw_config, {n}));\n' for n in cf) + "  return 0;\n}\n")
    subprocess.run([cc, "-I", str(ROOT / "include"), str(src), "-o", str(tmp_path / "offsets")], check=True, capture_output=True)
    out = subprocess.run([str(tmp_path / "offsets")], check=True, capture_output=True, text=True).stdout.split()
    assert [int(out[0]), int(out[1])] == [C.sizeof(lib.AdafactorTensor), C.sizeof(lib.AdamWConfig)]
    assert [int(x) for x in out[2:2 + len(tf)]] == [getattr(lib.AdafactorTensor, n).offset for n in tf]
    assert [int(x) for x in out[2 + len(tf):]] == [getattr(lib.AdamWConfig, n).offset for n in cf]
    assert [n for n, _t in lib.AdamWConfig._fields_][-len(cf):] == cf                     # appended at the end, in the header's order


def test_c_abi_argument_errors_for_algorithm_3():
    L = lib.load()
    cfg = lib.AdamWConfig()
    assert L.sdxl_adamw_default_config(C.byref(cfg)) == 0
    assert (cfg.clip_threshold, cfg.eps1, cfg.eps2, cfg.beta2t, cfg.rho, cfg.scale_parameter, cfg.use_beta1, cfg.tensors, cfg.n_tensors,
            cfg.af_state, cfg.af_scratch) == (0.0, 0.0, 0.0, 0.0, 0.0, 0, 0, None, 0, None, None)
    buf = (C.c_char * 512)()
    a16 = (C.addressof(buf) + 15) & ~15
    p16, odd = C.c_void_p(a16), C.c_void_p(a16 + 4)
    tab = (lib.AdafactorTensor * 2)()

    def good():
        cfg.algorithm, cfg.weight_decay, cfg.beta1 = 3, 0.0, 0.9
        cfg.clip_threshold, cfg.eps1, cfg.eps2, cfg.beta2t, cfg.rho, cfg.scale_parameter, cfg.use_beta1 = 1.0, 1e-30, 1e-3, 0.0, 1e-2, 1, 0
        cfg.tensors, cfg.n_tensors, cfg.af_state, cfg.af_scratch, cfg.ema = C.addressof(tab), 2, a16, a16, None
        for t, (off, rows, cols, numel, fac, so) in zip(tab, ((0, 2, 8, 16, 1, 0), (16, 1, 8, 5, 0, 12))):
            t.elem_off, t.rows, t.cols, t.numel, t.factored, t.state_off = off, rows, cols, numel, fac, so

    def refused(*what, **args):
        a = dict(p=p16, grad=p16, m=None, v=None, shift=p16, n=24, rand=None)
        a.update(args)
        rc = L.sdxl_adamw_bf16_step(a["p"], a["grad"], 0, a["m"], a["v"], a["shift"], a["n"], C.byref(cfg), None, a["rand"], None)
        msg = L.sdxl_last_error()
        assert rc == 1 and b"algorithm 3" in msg and all(w in msg for w in what), (what, rc, msg)

    cfg.algorithm = 3                                    # the default configuration: no table, no buffers, clip_threshold 0
    refused()
    cfg.algorithm = 4                                    # the message that lists the known algorithms names 3
    refused(b"algorithm 4")
    good(); refused(b"v must be NULL", v=p16)
    good(); refused(b"rand_inject", rand=p16)
    good(); refused(b"m must be", m=p16)                 # a first moment without use_beta1
    good(); cfg.use_beta1 = 1; refused(b"m must be")     # ... and use_beta1 without one
    for name in ("p", "grad", "shift"):
        good(); refused(b"missing", **{name: None})
        good(); refused(b"aligned", **{name: odd})
    good(); cfg.use_beta1 = 1; refused(b"aligned", m=odd)
    for name in ("af_state", "af_scratch"):
        good(); setattr(cfg, name, None); refused(b"missing")
        good(); setattr(cfg, name, a16 + 4); refused(b"aligned")
    good(); cfg.tensors = None; refused(b"missing")
    good(); cfg.ema, cfg.ema_one_minus_decay = a16 + 4, 0.5; refused(b"aligned")
    good(); refused(b"multiple of 8", n=28)
    for name, bad in (("clip_threshold", (0.0, -1.0, math.inf)), ("beta2t", (-0.1, 1.0, math.nan)), ("rho", (math.inf, math.nan)),
                      ("eps1", (-1e-30,)), ("eps2", (-1e-3,)), ("weight_decay", (-0.1,))):
        for x in bad:
            good(); setattr(cfg, name, x); refused(name[:4].encode())
    good(); cfg.use_beta1, cfg.beta1 = 1, 1.0; refused(b"beta1", m=p16)
    # the table: every message names the entry
    good(); tab[1].elem_off = 8; refused(b"entry 1", b"overlap")                     # overlapping
    good(); tab[0].elem_off, tab[1].elem_off = 16, 0; refused(b"entry 1", b"sorted", n=40)  # unsorted
    good(); refused(b"entry 1", b"past n", n=16)                                     # a range past n
    good(); tab[0].cols, tab[0].rows = 4, 4; refused(b"entry 0", b"multiple of 8")   # cols % 8
    good(); tab[1].numel = 0; refused(b"entry 1", b"numel")
    good(); tab[1].numel = 9; refused(b"entry 1", b"numel")
    good(); tab[0].elem_off = 4; refused(b"entry 0", b"multiple of 8")
    good(); tab[0].rows = 0; refused(b"entry 0")
    good(); tab[1].state_off = 13; refused(b"entry 1", b"state_off")
    good(); tab[0].factored = 2; refused(b"entry 0", b"factored")
    # an empty table is a step that does nothing
    good(); cfg.n_tensors = 0
    assert L.sdxl_adamw_bf16_step(p16, p16, 0, None, None, p16, 24, C.byref(cfg), None, None, None) == 0


# ---------------------------------------------------------------------------------------------- the bounds, tried on single defects
def _case(seed, rows, cols, numel, factored, zero_row=True):
    g0 = torch.Generator().manual_seed(seed)
    e = R.Entry(0, rows, cols, numel, factored, 0)
    mask = (torch.arange(rows * cols) < numel).reshape(rows, cols) if not factored else torch.ones(rows, cols, dtype=torch.bool)
    x = ((torch.randn(rows, cols, generator=g0) * 0.05).to(torch.bfloat16).float() * mask).numpy()
    gs = []
    for _k in range(2):
        g = torch.randn(rows, cols, generator=g0) * 3.0 * mask
        if zero_row and rows > 2:
            g[1] = 0                                     # a row without gradient: its statistic is eps1 alone
        gs.append(g.numpy())
    return e, x, gs


def _two_steps(e, x, gs, hp, order, mutant):
    """two steps of the float32 emulation, each checked against step64 on the emulation's own inputs: the largest used fraction per key"""
    state = {"R": np.zeros(e.rows, np.float32), "C": np.zeros(e.cols, np.float32)} if e.factored else {"v": np.zeros((e.rows, e.cols), np.float32)}
    m = np.zeros((e.rows, e.cols), np.float32)
    worst, prev_mean = {}, None
    for k in (1, 2):
        sc = hp.scalars(k)
        gr = gs[k - 1].astype(np.float32)
        s64 = {n: v.astype(np.float64) for n, v in state.items()}
        ref = R.step64(e, gr.astype(np.float64), x.astype(np.float64), s64, m.astype(np.float64), sc)
        bnd = R.bounds(e, ref, s64, m.astype(np.float64), sc)
        got = R.emulate32(e, gr, x, state, m, sc, order=order, mutant=mutant, prev_mean=prev_mean)
        got["pc"] = got["x"]
        for key, f in R.fractions(e, got, ref, bnd).items():
            worst[key] = max(worst.get(key, 0.0), f)
        state = {n: got[n].astype(np.float32) for n in state}
        prev_mean = got.get("mean")
        m = got["m"].astype(np.float32) if got["m"] is not None else m
        x = got["x"].astype(np.float32)
    return worst


MUTANT_CASES = {                                         # mutant -> (the case it shows on, hyper-parameters)
    "no_eps1": (dict(rows=37, cols=72, numel=37 * 72, factored=True), dict()),
    "cols_for_rows": (dict(rows=37, cols=72, numel=37 * 72, factored=True), dict()),
    "stale_mean": (dict(rows=37, cols=72, numel=37 * 72, factored=True), dict()),
    "numel_with_pads": (dict(rows=1, cols=1288, numel=1281, factored=False), dict()),
    "clip_below": (dict(rows=37, cols=72, numel=37 * 72, factored=True), dict(clip_threshold=4.0)),
    "no_eps2_floor": (dict(rows=37, cols=72, numel=37 * 72, factored=True), dict(eps=(1e-30, 1.0))),
    "decay_by_eta": (dict(rows=37, cols=72, numel=37 * 72, factored=True), dict(weight_decay=0.1, clip_threshold=0.25)),      # (clipped: eta_t < rho_t)
    "drop_last_row_block": (dict(rows=129, cols=248, numel=129 * 248, factored=True), dict()),
}


@pytest.mark.parametrize("mutant", list(R.MUTANTS))
def test_bounds_pass_a_reordered_float32_emulation_and_fail_each_single_defect(mutant):
    case, hyper = MUTANT_CASES[mutant]
    hp = R.Hyper(beta1=0.9, **hyper)
    e, x, gs = _case(11, **case)
    for order in ("pairwise", "reverse"):                # a correct emulation in either order stays inside every bound
        ok = _two_steps(e, x, gs, hp, order, None)
        assert ok and max(ok.values()) <= 1.0, (order, ok)
    with np.errstate(divide="ignore", invalid="ignore"):  # (a defect may divide by a zero statistic: that is how it shows)
        bad = _two_steps(e, x, gs, hp, "pairwise", mutant)
    print(f"{mutant}: clean {max(ok.values()):.3f} of the bound, defective {max(bad.values()):.3g}")
    assert max(bad.values()) > 1.0, bad
