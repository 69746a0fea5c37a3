"""The in-situ audit on the GPU: one training step, then EVERY op of the plan recomputed on the CPU from the operands it actually had.

tests/test_gpu_model.py and test_gpu_fullsize.py hold the composed step to aggregate bars (forward max|err| <= max(3 e_bf, 2e-2) max|ref|, gradients
rel-L2 <= 6e-2, cosine >= 0.995): a dropped row of a weight-gradient sum, a stale pad row, a wrong addend, a shifted column slice or a wrong eps /
split / accumulate flag handed to a kernel all pass them.  Here the plan map (sdxl_debug_plan_op) says where every op reads and writes, the
workspace and both arenas are copied to the CPU once after a synchronised forward_loss + zero_grads + backward, and tests/_insitu.py holds every
output of every op to the per-element bounds of the op tests.  The audit launches nothing but the ordinary step.

Cases: the smallest at which the engine's decisions still vary (the [insitu-reach] line of each says what it reached)."""
import ctypes as C
import dataclasses

import pytest
import torch

import sdxl_amd  # noqa: F401
from oracle import loss_ref as R
from oracle import unet_ref as U
from sdxl_amd import lib
from sdxl_amd import unet as NU

import _insitu as IS
from test_gpu_model import make_inputs

pytestmark = pytest.mark.gpu


def native_cfg(c: U.UNetConfig):
    return NU.make_config(block_out_channels=c.block_out_channels, transformer_layers=c.transformer_layers_per_block,
                          layers_per_block=c.layers_per_block, cross_attention_dim=c.cross_attention_dim,
                          addition_time_embed_dim=c.addition_time_embed_dim, pooled_dim=c.pooled_dim)


TINY = U.tiny_config()
# narrow depth, real widths: LayerNorm over 640 / 1280, GroupNorm with 10 / 20 / 40 / 60 / 80 channels a group, GEGLU widths 5120 / 10240, the real
# conditioning widths (cross 2048, pooled 1280, time ids 256)
REAL = dataclasses.replace(U.UNetConfig(), transformer_layers_per_block=(0, 1, 1))
# one resnet a level, widths (64, 128, 384): at 16 samples of 32 x 32 the 384-wide level has 1024 rows, where the GEGLU projection's weight gradient
# ([3072][384]: 72 tiles of 128 x 160, a split reduction) is the smallest that the plan launches in groups, and the 128-wide level's self-attention (256 keys,
# 64 (batch, head) pairs: no query split) takes the fused backward with Delta from the out-projection's dgrad epilogue
GROUPED = dataclasses.replace(TINY, block_out_channels=(64, 128, 384), layers_per_block=1, transformer_layers_per_block=(0, 1, 1))


def make_net(cfg):
    net = NU.NativeUNet(native_cfg(cfg))
    net.load_state_dict(U.synth_weights(cfg, seed=0))
    return net


@pytest.fixture(scope="module")
def tiny():
    net = make_net(TINY)
    yield TINY, net
    net.close()


@pytest.fixture(scope="module")
def real():
    net = make_net(REAL)
    yield REAL, net
    net.close()


@pytest.fixture(scope="module")
def grouped():
    net = make_net(GROUPED)
    yield GROUPED, net
    net.close()


def forward(net, cfg, B, H, W, method, seed, **loss_kw):
    """one forward_loss; x["loss"] keeps the caller's side of the loss seam (the arrays and options as handed over) for the audit.
    loss_kw: forward_loss's optional loss arguments (sample_weights, tag_weights, huber_c, loss_type, per_sample_loss, loss_mask, mask_norm, noise_in,
    input_cond)"""
    x = make_inputs(cfg, B, H, W, seed=seed)
    if method == "ddpm":
        ts = torch.tensor([700, 420, 133, 866][:B]) if B <= 4 else (torch.arange(B) * 61 + 17) % 1000
        sig, tt = R.karras_sigmas()[ts], ts.float()
    else:
        sig = tt = R.sample_logit_normal_from_z(x["z"])
        assert B == 1 or len({float(v) for v in sig}) == B, "the samples must differ in t"
    net.forward_loss(method, x["lat"], x["noise"], sig, tt, x["ehs"], x["pooled"], x["tid"], **loss_kw)
    hc = loss_kw.get("huber_c")
    x["loss"] = dict(method=method, lat=x["lat"], noise=x["noise"], sig=sig, noise_in=loss_kw.get("noise_in"), tag=loss_kw.get("tag_weights"),
                     sw=loss_kw.get("sample_weights"), hc=hc if torch.is_tensor(hc) else None, c=hc if isinstance(hc, float) else 0.0,
                     mask=loss_kw.get("loss_mask"), cond=loss_kw.get("input_cond"), loss_type=loss_kw.get("loss_type", "l2"),
                     mask_norm=loss_kw.get("mask_norm", "mean"), per_sample=loss_kw.get("per_sample_loss", False))
    return x


def snapshot(net, x, g0=None, accumulate=False, grad_scale=1.0):
    torch.cuda.synchronize()
    ops, tail = lib.plan_map(net.h)
    tail["pooled_in"] = x["pooled"]      # the caller's array: the audit holds aug_in's first half to its bf16 bits
    tail["loss"] = dict(plan=lib.plan_loss(net.h), caller=x["loss"], grad_scale=grad_scale)      # the loss seam: _insitu.audit_seam
    img = IS.Image(net.workspace.cpu()[:tail["workspace_bytes"]], net.weights.cpu(), net.grads.cpu(), g0, accumulate)
    return ops, tail, img


def workspace_bytes(net, B, H, W):
    need = C.c_size_t()
    lib.check(net.L.sdxl_plan(net.h, B, H, W, 77, C.byref(need)), "sdxl_plan")
    return need.value


def report(tag, ops, results, net):
    for kind, (worst, n, elems) in sorted(IS.summarize(results).items()):
        print(f"[insitu] {tag} {kind}: worst err / allowed {worst:.4g} over {n} outputs, {elems} elements")
    print(f"[insitu-reach] {tag}: {'; '.join(IS.reach(ops))}")
    # (kinds=(): which kinds have an audited instance of their own is judged over the module's cases, test_every_kind_... below)
    problems, taken = IS.coverage(ops, results, net.param_ranges(), kinds=())
    print(f"[insitu-coverage] {tag}: {len(ops)} ops, {len(results)} outputs, {len(net.param_ranges())} parameter tensors; omitted: "
          f"{sorted({(k, r) for _, k, r in taken}) or 'nothing'}; problems: {len(problems)}")
    bad = IS.failures(results)
    assert not bad, f"{tag}: {len(bad)} outputs outside their bounds:\n" + "\n".join(bad[:20])
    assert not problems, f"{tag}: coverage:\n" + "\n".join(problems[:20])


def step_and_audit(net, cfg, B, H, W, method, seed=11):
    before = workspace_bytes(net, B, H, W)
    x = forward(net, cfg, B, H, W, method, seed)
    net.zero_grads()
    net.backward(grad_scale=1.0, first_micro=True)
    ops, tail, img = snapshot(net, x)
    # the plan map reserved nothing and moved nothing: the plan's size is what it was before the hooks were called
    assert workspace_bytes(net, B, H, W) == before == tail["workspace_bytes"]
    assert all(bool(torch.isfinite(torch.tensor(v))) for v in net.read_loss()[:1])
    return ops, tail, img


_DONE = {}      # case -> (ops, results): each case's step and audit run once in the module


def case(tag, net, cfg, B, H, W, method):
    if tag not in _DONE:
        ops, tail, img = step_and_audit(net, cfg, B, H, W, method)
        _DONE[tag] = (ops, IS.audit(ops, tail, img))
    return _DONE[tag]


TINY_CASES = [(2, 16, 16, "ddpm"), (3, 12, 20, "flow_matching")]


@pytest.mark.parametrize("B,H,W,method", TINY_CASES, ids=["2x16x16-ddpm", "3x12x20-flow"])
def test_every_op_of_the_tiny_step(tiny, B, H, W, method):
    """256 / 64 / 16 rows a sample, everything tile-aligned; and 720 / 180 / 45 rows with three different t: ragged everywhere, odd batch seams,
    the 231 prompt rows padded to 256 (pad rows of both weight-gradient operands)"""
    cfg, net = tiny
    tag = f"tiny {B}x{H}x{W} {method}"
    ops, results = case(tag, net, cfg, B, H, W, method)
    report(tag, ops, results, net)


@pytest.mark.parametrize("B,H,W", [(1, 16, 16), (2, 8, 12)], ids=["1x16x16", "2x8x12"])
def test_every_op_at_the_real_widths(real, B, H, W):
    """LayerNorm widths 640 / 1280, GEGLU widths 5120 / 10240 with the group the plan picks, small-M split-K forward / dgrad, the K % 128 Delta
    predicate; the float64 references are at most 256 rows tall"""
    cfg, net = real
    tag = f"real-width {B}x{H}x{W}"
    ops, results = case(tag, net, cfg, B, H, W, "ddpm")
    report(tag, ops, results, net)


def test_every_op_where_weight_gradients_are_grouped(grouped):
    """the smallest shape at which the plan groups weight gradients and fuses Delta into the out-projection's dgrad (GROUPED above)"""
    cfg, net = grouped
    B, H, W = 16, 32, 32
    tag = f"grouped {B}x{H}x{W}"
    ops, results = case(tag, net, cfg, B, H, W, "flow_matching")
    got = IS.reach(ops)
    assert "grouped wgrad" in got and "Delta fused" in got and "Delta pass" in got and "self attention: fused" in got, got
    report(tag, ops, results, net)


def test_every_kind_has_an_audited_instance_of_its_own(tiny, real, grouped):
    """over the module's product cases (each run once, shared with the tests above): every op kind has a forward and a backward output of its
    OWN audited -- a listed omission and a result borrowed from another op's audit do not count.  The one exception is stated, not hidden: the
    shipped plan fuses every up-sampler into its convolution, so the stand-alone nearest-2x backward is never launched; its gradient is audited
    inside the up-convolution's dgrad (dx_in_upconv, which must then be there) and, stand-alone, by the diagnostics case below (knob 2 = 64)."""
    runs = [case(f"tiny {B}x{H}x{W} {m}", tiny[1], tiny[0], B, H, W, m) for B, H, W, m in TINY_CASES]
    runs += [case(f"real-width {B}x{H}x{W}", real[1], real[0], B, H, W, "ddpm") for B, H, W in ((1, 16, 16), (2, 8, 12))]
    runs += [case("grouped 16x32x32", grouped[1], grouped[0], 16, 32, 32, "flow_matching")]
    fwd, bwd = set(), set()
    for ops, results in runs:
        f, b = IS.audited_kinds(ops, results)
        fwd |= f
        bwd |= b
    print(f"[insitu-kinds] forward: {sorted(fwd)}; backward: {sorted(bwd)}")
    assert fwd == set(lib.PLAN_KINDS), sorted(set(lib.PLAN_KINDS) - fwd)
    assert bwd == set(lib.PLAN_KINDS) - {"embed_in", "upsample"}, sorted(bwd)      # (embed_in: inputs only, no gradient)
    assert all(any(r.kind == "upsample" and r.role == "dx_in_upconv" and r.ok for r in results) for _, results in runs)


def test_plan_map_refuses_bad_arguments(tiny):
    """a bad index and a null pointer return 1 with a message, like every hook; nothing is written"""
    cfg, net = tiny
    net.plan(2, 16, 16)
    L = net.L
    n = C.c_int()
    lib.check(L.sdxl_debug_plan_num_ops(net.h, C.byref(n)))
    d = lib.PlanOpDesc()
    d.kind = -5
    sz, tsz = C.sizeof(lib.PlanOpDesc), C.sizeof(lib.PlanTail)
    for i in (-1, n.value):
        assert L.sdxl_debug_plan_op(net.h, i, C.byref(d), sz) == 1 and b"out of range" in L.sdxl_last_error() and d.kind == -5
    for rc in (L.sdxl_debug_plan_num_ops(net.h, None), L.sdxl_debug_plan_op(net.h, 0, None, sz), L.sdxl_debug_plan_tail(net.h, None, tsz),
               L.sdxl_debug_plan_loss(net.h, None, C.sizeof(lib.PlanLoss))):
        assert rc == 1 and b"null output" in L.sdxl_last_error()
    assert L.sdxl_debug_plan_loss(net.h, C.byref(lib.PlanLoss()), C.sizeof(lib.PlanLoss) + 8) == 1 and b"bytes" in L.sdxl_last_error()
    pl = lib.plan_loss(net.h)
    assert pl["loss_part_off"] is not None and pl["ps_loss_off"] is not None and pl["in_lat_off"] is not None and pl["in_cond_off"] is None
    assert pl["ps_slots"] == 2 and pl["part_floats"] == (6 + 2 * 2) * 2
    # a struct of another size is refused before it is written to
    assert L.sdxl_debug_plan_op(net.h, 0, C.byref(d), sz - 8) == 1 and b"bytes" in L.sdxl_last_error() and d.kind == -5
    assert L.sdxl_debug_plan_tail(net.h, C.byref(lib.PlanTail()), tsz + 8) == 1 and b"bytes" in L.sdxl_last_error()
    ops, tail = lib.plan_map(net.h)
    assert len(ops) == n.value and ops[0]["kind"] == "embed_in" and (tail["B"], tail["H"], tail["W"], tail["ctx"]) == (2, 16, 16, 77)
    assert tail["pred"]["goff"] is not None and tail["x_in"]["goff"] is None


def test_second_micro_step_accumulates(tiny):
    """first_micro = False on other inputs: every weight / bias / norm gradient is the arena image from before the step + this step's
    contribution, in fp32 (the accumulate side of every parameter-gradient path, in place)"""
    cfg, net = tiny
    B, H, W = 2, 16, 16
    forward(net, cfg, B, H, W, "ddpm", 11)
    net.zero_grads()
    net.backward(grad_scale=1.0, first_micro=True)
    torch.cuda.synchronize()
    g0 = net.grads.cpu().clone()
    assert int(g0.ne(0).sum()) > 0.9 * sum(n for _, n in net.param_ranges().values())
    x = forward(net, cfg, B, H, W, "ddpm", 12)
    net.backward(grad_scale=1.0, first_micro=False)
    ops, tail, img = snapshot(net, x, g0=g0, accumulate=True)
    results = [r for r in IS.audit(ops, tail, img) if r.role in IS.PARAM_ROLES and r.kind in IS.PARAM_KINDS]
    assert len(results) >= len(ops) // 2
    for kind, (worst, n, elems) in sorted(IS.summarize(results).items()):
        print(f"[insitu] second micro-step {kind}: worst err / allowed {worst:.4g} over {n} parameter gradients, {elems} elements")
    bad = IS.failures(results)
    assert not bad, f"{len(bad)} accumulated gradients outside their bounds:\n" + "\n".join(bad[:20])


# ------------------------------------------------------------------------------------------------ the loss seam in place
def seam_kw(B, H, W, which, seed=0):
    g = torch.Generator().manual_seed(900 + seed)
    if which == "weights":      # sample_weights with a zero, tag_weights, per-sample losses, smooth_l1 with per-sample c
        sw = torch.rand(B, generator=g) + 0.5
        sw[1] = 0.0
        return dict(sample_weights=sw, tag_weights=torch.rand(B, generator=g) + 0.5, per_sample_loss=True, loss_type="smooth_l1",
                    huber_c=torch.rand(B, generator=g) * 0.5 + 0.1)
    if which == "mask":         # a fractional mask under masked_mean and an input noise of its own
        import _loss_elem as LE
        return dict(loss_mask=LE.fractional_mask(B, H, W, seed=901 + seed, empty=None), mask_norm="masked_mean", per_sample_loss=True,
                    noise_in=torch.randn(B, 4, H, W, generator=g))
    raise KeyError(which)


def seam_step(net, cfg, B, H, W, method, seed, first_micro=True, g0=None, **kw):
    x = forward(net, cfg, B, H, W, method, seed, **kw)
    if first_micro:
        net.zero_grads()
    net.backward(grad_scale=0.5, first_micro=first_micro)
    return snapshot(net, x, g0=g0, accumulate=not first_micro, grad_scale=0.5)


def seam_report(tag, ops, tail, img, staged, net):
    results = IS.audit(ops, tail, img)
    seam = [r for r in results if r.kind == IS.SEAM_KIND]
    print(f"[insitu-seam] {tag}: staged {tail['loss']['plan']['staged']}; " + ", ".join(f"{r.role} {r.ratio:.3g}" for r in seam))
    assert tail["loss"]["plan"]["staged"] == staged and {r.role for r in seam} >= set(IS.SEAM_ROLES) | ({"staged"} if staged else set())
    report(tag, ops, results, net)
    return results


def test_loss_seam_with_weights_and_per_sample_huber(tiny):
    cfg, net = tiny
    B, H, W = 3, 12, 20
    ops, tail, img = seam_step(net, cfg, B, H, W, "flow_matching", 21, **seam_kw(B, H, W, "weights"))
    results = seam_report(f"seam {B}x{H}x{W} flow weights smooth_l1", ops, tail, img, 0, net)
    assert any(r.role == "L_b" for r in results)


def test_loss_seam_with_a_masked_mean_and_an_input_noise(tiny):
    cfg, net = tiny
    B, H, W = 2, 16, 16
    ops, tail, img = seam_step(net, cfg, B, H, W, "ddpm", 22, **seam_kw(B, H, W, "mask"))
    results = seam_report(f"seam {B}x{H}x{W} ddpm masked_mean noise_in", ops, tail, img, 0, net)
    assert any(r.role == "mnorm" for r in results) and any(r.role == "L_b" for r in results)


def test_loss_seam_with_input_cond_on_the_nine_channel_unet():
    """the tiny UNet of test_gpu_input_cond.py with in_channels = 9 (Cs = 16).  The library takes latent sizes that are multiples of 4 only, so the
    13 x 10 of the op tests cannot run through a UNet: 12 x 12 is the nearest size whose blocks straddle the samples (HW = 144)"""
    cfg = dataclasses.replace(TINY, in_channels=9)
    net = NU.NativeUNet(NU.make_config(in_channels=9, block_out_channels=cfg.block_out_channels, transformer_layers=cfg.transformer_layers_per_block,
                                       layers_per_block=cfg.layers_per_block, cross_attention_dim=cfg.cross_attention_dim,
                                       addition_time_embed_dim=cfg.addition_time_embed_dim, pooled_dim=cfg.pooled_dim))
    try:
        net.load_state_dict(U.synth_weights(cfg, seed=0))
        B, H, W = 2, 12, 12
        cond = torch.randn(B, 5, H, W, generator=torch.Generator().manual_seed(23))
        ops, tail, img = seam_step(net, cfg, B, H, W, "ddpm", 23, input_cond=cond)
        assert tail["x_in"]["cols"] == 16
        seam_report(f"seam {B}x{H}x{W} ddpm input_cond 9 channels", ops, tail, img, 0, net)
    finally:
        net.close()


def test_loss_seam_in_graph_mode_reads_the_staged_copies(tiny):
    """the weights case again under hipGraph replay: the third call with one key is a replay; every call gets other arrays in other allocations,
    and the audit of the third holds each staged copy to the caller's array and recomputes from the copies"""
    cfg, net = tiny
    B, H, W = 3, 12, 20
    net.set_graph_mode(True)
    try:
        for i in range(3):
            ops, tail, img = seam_step(net, cfg, B, H, W, "flow_matching", 24 + i, **seam_kw(B, H, W, "weights", seed=i))
    finally:
        net.set_graph_mode(False)
    seam_report(f"seam {B}x{H}x{W} flow weights smooth_l1, graph replay", ops, tail, img, 1, net)


def test_loss_seam_on_an_accumulating_micro_step(tiny):
    cfg, net = tiny
    B, H, W = 3, 12, 20
    seam_step(net, cfg, B, H, W, "flow_matching", 27, **seam_kw(B, H, W, "weights", seed=3))
    g0 = net.grads.cpu().clone()
    ops, tail, img = seam_step(net, cfg, B, H, W, "flow_matching", 28, first_micro=False, g0=g0, **seam_kw(B, H, W, "weights", seed=4))
    seam_report(f"seam {B}x{H}x{W} flow weights smooth_l1, first_micro = False", ops, tail, img, 0, net)


DIAG_CASES = [
    # knobs, config, shape, method, what the reach line / the audited kinds must show
    ("ln-epilogue", {26: 1, 35: 2}, "TINY", (3, 12, 20), "flow_matching", ["ln_mode 1"]),
    ("pipelined-attention", {26: 1, 35: 2}, "GROUPED", (16, 32, 32), "flow_matching", ["self attention: pipelined", "Delta fused"]),
    ("plain-upsample", {2: 64}, "TINY", (3, 12, 20), "flow_matching", []),
]


@pytest.mark.diag
@pytest.mark.parametrize("name,knobs,which,shape,method,must_reach", DIAG_CASES, ids=[c[0] for c in DIAG_CASES])
def test_plans_of_the_diagnostics_build(name, knobs, which, shape, method, must_reach):
    """Plans that otherwise run only in hook tests, audited in place.  knob 26 = 1: the LayerNorm backward inside its consumer's dgrad epilogue
    (the ragged tiny case).  knob 35 = 2: the pipelined self-attention backward wherever it applies, which is from 256 keys on -- the 128-wide
    level of the grouped case (the tiny case has 60 keys: the knob changes nothing there).  knob 2 = 64: no up-convolution, so the nearest-2x
    forward and its stand-alone backward, which the shipped plan never launches, run and are audited as ops of their own."""
    L = lib.load()
    cfg = {"TINY": TINY, "GROUPED": GROUPED}[which]
    net = None
    for k, v in knobs.items():
        lib.check(L.sdxl_set_knob(k, v))
    try:
        net = make_net(cfg)
        ops, tail, img = step_and_audit(net, cfg, *shape, method)
        torch.cuda.synchronize()
        err = C.c_uint(99)
        lib.check(L.sdxl_ln_error(C.byref(err)))
        assert err.value == 0, f"a LayerNorm-backward epilogue gave up its in-launch meeting (error word {err.value})"
        results = IS.audit(ops, tail, img)
        got = IS.reach(ops)
        assert all(f in got for f in must_reach), (must_reach, got)
        if name == "plain-upsample":
            fwd, bwd = IS.audited_kinds(ops, results)
            assert "upsample" in fwd and "upsample" in bwd and "up2" not in got and "up2 + wgrad" not in got, (sorted(bwd), got)
        report(f"{which.lower()} {'x'.join(map(str, shape))} knobs {knobs}", ops, results, net)
    finally:
        for k in knobs:
            lib.check(L.sdxl_set_knob(k, 0))
        if net is not None:
            net.close()
