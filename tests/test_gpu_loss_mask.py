"""The loss mask, its two normalisations and the separate input noise of the HIP loss kernels (csrc/loss.hip), through the C ABI
`sdxl_op_loss` on the `Case` pattern of test_gpu_loss_ext.py, then through the whole step on the tiny UNet.

The reference is tests/_loss_mask_ref.py in float64 on the SAME bf16-rounded prediction, fp32 target and MinSNR weight.  Bars are
those of test_gpu_loss_ext.py: losses and L_b 1e-5 relative; dpred max error <= 2^-8 of the largest reference magnitude and median
relative error <= 2^-8, both over the elements with m > 0 only (where m = 0 the device value must be an exact zero, which would
otherwise pull the median down).

Shapes: B = 4 at 13 x 10 (HW = 130: every block straddles samples), 64 x 64 and 104 x 152 (HW = 61.75 blocks).  Mask values come
from {0, 1/4, 1/2, 1}, so M_b is exact in fp32 in any summation order: sample 0 is all zero, sample 1 all one, sample 2 has a
rectangle of ones, sample 3 is random."""
import ctypes as C

import pytest
import torch

import sdxl_amd  # noqa: F401
from oracle import loss_ref as R
from oracle import unet_ref as U
from sdxl_amd import lib
from sdxl_amd import unet as NU

import _loss_ext_ref as X
import _loss_mask_ref as MR
from _gradparity import GradParity, compare_autograd
from test_gpu_loss_ext import (DEV, DPRED_BAR, LOSS_RTOL, METHODS, TINY_GRAD_BAR, TINY_TS, Case, _dev, _st, _tiny_step, bits,
                               check_loss, check_per_sample, from_rows8, make, make_inputs, tiny_native_cfg)

pytestmark = pytest.mark.gpu
SHAPES = [(4, 13, 10), (4, 64, 64), (4, 104, 152)]
NORMS = ["mean", "masked_mean"]


@pytest.fixture(scope="module")
def L():
    assert torch.cuda.is_available()
    return lib.load()


def make_mask(B, H, W, seed):
    g = torch.Generator().manual_seed(seed)
    m = torch.tensor([0.0, 0.25, 0.5, 1.0])[torch.randint(0, 4, (B, H, W), generator=g)]
    m[0] = 0.0
    m[1] = 1.0
    m[2] = 0.0
    m[2, H // 4:H // 4 + H // 2, W // 3:W // 3 + W // 2] = 1.0
    return m


class MaskCase(Case):
    """Case with the full sdxl_loss_config: `mask` [B,H,W], `mask_norm`, `noise_in` [B,4,H,W]"""

    def __init__(self, L, method, lat, noise, sig, mask=None, mask_norm="mean", noise_in=None, **kw):
        super().__init__(L, method, lat, noise, sig, **kw)
        self.keep += [_dev(mask), _dev(noise_in)]
        ext = lib.LossConfigExt(*[getattr(self.lc, f[0]) for f in lib.LossConfig._fields_])
        ext.loss_type |= lib.LOSS_EXT
        ext.mask_norm = lib.MASK_NORMS[mask_norm]
        ext.loss_mask = None if mask is None else self.keep[-2].data_ptr()
        ext.noise_in = None if noise_in is None else self.keep[-1].data_ptr()
        self.lc = ext

    def prepare(self):
        """phase 0: the UNet input [B,4,H,W] bf16"""
        rows = torch.full((self.B * self.H * self.W, 8), -3.0, dtype=torch.bfloat16, device=DEV)
        lib.check(self.L.sdxl_op_loss(C.byref(self.lc), C.byref(self.b), C.c_void_p(rows.data_ptr()), None, None, 1.0, None, 0, _st()))
        assert int(bits(rows[:, 4:]).ne(0).sum()) == 0
        return from_rows8(rows, self.B, self.H, self.W)


def run(cs, pred, scale=1.0):
    """(out, L_b, dpred bf16 [B,4,H,W]) of phases 1 and 2"""
    out = torch.zeros(8, dtype=torch.float32, device=DEV)
    dp = torch.empty(cs.B * cs.H * cs.W, 8, dtype=torch.bfloat16, device=DEV)
    lib.check(cs.raw(pred, 1, out=out))
    lib.check(cs.raw(pred, 2, scale=scale, out=out, dp=dp))
    return out.cpu(), None if cs.ps is None else cs.ps.cpu().clone(), from_rows8(dp, cs.B, cs.H, cs.W)


def same_bits(a, b):
    return all(torch.equal(bits(x), bits(y)) for x, y in zip(a, b))


# ------------------------------------------------------------------------------------------------ 1. m = 1 changes no bit
@pytest.mark.parametrize("B,H,W", SHAPES)
@pytest.mark.parametrize("method", ["ddpm", "flow_matching"])
def test_ones_mask_with_mean_is_bitwise_the_unmasked_loss(L, method, B, H, W):
    lat, noise, sig, target, w, pred = make(method, B, H, W, seed=700 + H)
    sw = torch.tensor([0.7, 1.3, 2.0, 0.1])
    base = run(Case(L, METHODS[method], lat, noise, sig, sw=sw, per_sample=True), pred, 0.5)
    ones = run(MaskCase(L, METHODS[method], lat, noise, sig, mask=torch.ones(B, H, W), sw=sw, per_sample=True), pred, 0.5)
    assert same_bits(ones, base)
    # the flag alone (no mask, no noise_in) is the short struct's call
    flag = run(MaskCase(L, METHODS[method], lat, noise, sig, sw=sw, per_sample=True), pred, 0.5)
    assert same_bits(flag, base)
    assert float(base[2].float().abs().max()) > 0.0
    # without the per-sample output and weights too (the NULL branches)
    assert same_bits(run(MaskCase(L, METHODS[method], lat, noise, sig, mask=torch.ones(B, H, W)), pred)[::2],
                     run(Case(L, METHODS[method], lat, noise, sig), pred)[::2])


# ------------------------------------------------------------------------------------------------ 2. noise_in
@pytest.mark.parametrize("B,H,W", SHAPES)
@pytest.mark.parametrize("method", ["ddpm", "flow_matching"])
def test_noise_in_reaches_the_input_only(L, method, B, H, W):
    lat, noise, sig, target, w, pred = make(method, B, H, W, seed=800 + H)
    nin = noise + 0.1 * torch.randn(noise.shape, generator=torch.Generator().manual_seed(3))
    mask = make_mask(B, H, W, seed=4)
    for kw in (dict(), dict(mask=mask, mask_norm="masked_mean")):
        without = MaskCase(L, METHODS[method], lat, noise, sig, per_sample=True, **kw)
        with_in = MaskCase(L, METHODS[method], lat, noise, sig, noise_in=nin, per_sample=True, **kw)
        assert same_bits(run(with_in, pred, 0.5), run(without, pred, 0.5))      # phases 1 and 2 never read it
    got = with_in.prepare()
    assert torch.equal(bits(got), bits(MR.prepare(method, lat, nin, sig)))
    plain = without.prepare()
    assert torch.equal(bits(plain), bits(MR.prepare(method, lat, noise, sig))) and not torch.equal(bits(plain), bits(got))


# ------------------------------------------------------------------------------------------------ 3. against float64
def check_masked_dpred(what, got_bf16, want, mask):
    live = (mask > 0).unsqueeze(1).expand_as(want)
    assert int(bits(got_bf16)[~live].ne(0).sum()) == 0, what                  # m = 0: an exact zero, bit for bit
    err = (got_bf16.double() - want).abs()[live]
    ref = want[live].abs()
    mx, med = float(err.max()) / float(ref.max()), float((err / ref.clamp_min(1e-30)).median())
    print(f"[loss-mask] {what}: dpred over m > 0 max err / max|ref| {mx:.2e}, median rel {med:.2e} (bar {DPRED_BAR:.2e})")
    assert mx <= DPRED_BAR and med <= DPRED_BAR, (what, mx, med)


@pytest.mark.parametrize("B,H,W", SHAPES)
@pytest.mark.parametrize("loss_type", ["l2", "huber"])
@pytest.mark.parametrize("norm", NORMS)
@pytest.mark.parametrize("method", ["ddpm", "flow_matching"])
def test_masked_loss_against_float64(L, method, norm, loss_type, B, H, W):
    lat, noise, sig, target, w, pred = make(method, B, H, W, seed=900 + H)
    mask = make_mask(B, H, W, seed=5 + W)
    g = torch.Generator().manual_seed(6)
    sw, tag = torch.rand(B, generator=g) * 2.0 + 0.05, torch.rand(B, generator=g) + 0.5
    c = 0.3
    kw = dict(mask=mask, mask_norm=norm, sw=sw, tag=tag, loss_type=lib.LOSS_TYPES[loss_type], c=c, per_sample=True)
    first = run(MaskCase(L, METHODS[method], lat, noise, sig, **kw), pred, 0.25)
    again = run(MaskCase(L, METHODS[method], lat, noise, sig, **kw), pred, 0.25)
    assert same_bits(first, again)                                             # fixed-order sums: the same bits every time
    out, per, dp = first
    p64, t64, w64 = pred.double(), target.double(), w.double()
    args = (p64, t64, w64, mask.double(), norm, sw.double(), loss_type, c)
    what = f"{method} {norm} {loss_type} {B}x{H}x{W}"
    check_loss(what, float(out[0]), float(MR.loss(*args, tag.double())))
    want_per = MR.per_sample_loss(*args)
    assert float(per[0]) == 0.0 and float(want_per[0]) == 0.0                  # the empty sample
    check_per_sample(what, per, want_per)
    check_masked_dpred(what, dp, MR.dpred(*args, tag.double(), 0.25), mask)
    assert float(dp[1:].float().abs().max()) > 0.0
    # out[0] = out[1] / numel * tm holds in both normalisations; the gate is the tag mean; out[2..6] ignore the mask
    tm = float(tag.double().mean())
    assert abs(float(out[0]) - float(out[1]) / pred.numel() * tm) <= 1e-5 * float(out[0])
    assert float(out[7]) == pytest.approx(tm, rel=1e-6)
    plain = run(Case(L, METHODS[method], lat, noise, sig, sw=sw, tag=tag, loss_type=lib.LOSS_TYPES[loss_type], c=c), pred, 0.25)[0]
    assert torch.equal(bits(out[2:7]), bits(plain[2:7]))


@pytest.mark.parametrize("norm", NORMS)
def test_masked_pixels_stay_zero_where_the_difference_is_not_finite(L, norm):
    B, H, W = 4, 13, 10
    lat, noise, sig, target, w, pred = make("flow_matching", B, H, W, seed=950)
    mask = make_mask(B, H, W, seed=7)
    pred = pred.clone()
    pred[0, 1, 3, 3] = float("inf")                                            # in the empty sample (M_b = 0)
    out, per, dp = run(MaskCase(L, 1, lat, noise, sig, mask=mask, mask_norm=norm, per_sample=True), pred)
    assert int(bits(dp)[(mask == 0).unsqueeze(1).expand_as(dp)].ne(0).sum()) == 0
    if norm == "masked_mean":                                                  # L_b = 0 when M_b = 0, whatever the sample holds
        assert float(per[0]) == 0.0 and float(out[7]) == 1.0 and float(dp[1].float().abs().max()) > 0.0


def test_bad_mask_arguments_launch_nothing(L):
    lat, noise, sig, target, w, pred = make("ddpm", 4, 13, 10, seed=9)
    out = torch.full((8,), -3.0, dtype=torch.float32, device=DEV)
    dp = torch.full((4 * 130, 8), -3.0, dtype=torch.bfloat16, device=DEV)
    for loss_type, norm, match in ((lib.LOSS_EXT | 7, 0, "loss_type"), (0x200, 0, "loss_type"), (lib.LOSS_EXT, 2, "mask_norm")):
        cs = MaskCase(L, 0, lat, noise, sig, mask=torch.ones(4, 13, 10), per_sample=True)
        cs.lc.loss_type, cs.lc.mask_norm = loss_type, norm
        for phase in (1, 2):
            assert cs.raw(pred, phase, out=out, dp=dp) == 1
            assert match in L.sdxl_last_error().decode()
        torch.cuda.synchronize()
        assert float(out.min()) == float(out.max()) == -3.0 and float(dp.float().min()) == float(dp.float().max()) == -3.0
        assert float(cs.ps.min()) == float(cs.ps.max()) == -7.0


# ------------------------------------------------------------------------------------------------ 4. the whole path, tiny UNet
@pytest.fixture(scope="module")
def tiny():
    cfg = U.tiny_config()
    w = U.synth_weights(cfg, seed=0)
    net = NU.NativeUNet(tiny_native_cfg(cfg))
    net.load_state_dict(w)
    yield cfg, w, net
    net.set_graph_mode(False)
    net.close()


@pytest.mark.parametrize("norm", NORMS)
def test_masked_step_every_gradient_matches_oracle(tiny, norm):
    cfg, w, net = tiny
    B, H, W = 4, 16, 16
    x = make_inputs(cfg, B, H, W, seed=81)
    mask = make_mask(B, H, W, seed=8)
    out, per, _ = _tiny_step(net, x, loss_mask=mask, mask_norm=norm, per_sample_loss=True)
    for t in w.values():
        t.grad = None
        t.requires_grad_(True)
    try:
        sig = R.karras_sigmas()[TINY_TS]
        pred = U.unet_forward(w, R.add_noise(x["lat"], x["noise"], sig), TINY_TS, x["ehs"], x["pooled"], x["tid"], cfg)
        target, mw = X.target_and_weight("ddpm", x["lat"], x["noise"], sig)
        ref = MR.loss(pred, target, mw, mask, norm)
        ref_per = MR.per_sample_loss(pred.detach(), target, mw, mask, norm)
        check_loss(f"tiny {norm}", out[0], float(ref.detach()), rtol=LOSS_RTOL)
        assert float(per[0]) == 0.0 and float(ref_per[0]) == 0.0
        check_per_sample(f"tiny {norm}", per[1:], ref_per[1:], rtol=LOSS_RTOL)
        par = GradParity(f"tiny ddpm mask {norm} {B}x{H}x{W}")
        compare_autograd(par, ref, w, lambda k: net.export(k, grad=True))
    finally:
        for t in w.values():
            t.grad = None
            t.requires_grad_(False)
    par.check(TINY_GRAD_BAR, expect=net.param_shapes())


def test_ones_mask_leaves_the_gradient_arena_bitwise_and_graph_replay_follows_the_mask(tiny):
    cfg, w, net = tiny
    B, H, W = 4, 16, 16
    x = make_inputs(cfg, B, H, W, seed=82)
    ones, ma, mb = torch.ones(B, H, W), make_mask(B, H, W, seed=9), make_mask(B, H, W, seed=10).flip(0)
    nin = x["noise"] + 0.1 * torch.randn(x["noise"].shape, generator=torch.Generator().manual_seed(11))
    net.set_graph_mode(False)
    out0, _, g0 = _tiny_step(net, x)
    out1, per1, g1 = _tiny_step(net, x, loss_mask=ones, per_sample_loss=True)
    assert out0 == out1 and torch.equal(bits(g0), bits(g1))
    eager = {}
    for name, m in (("a", ma), ("b", mb)):
        eager[name] = _tiny_step(net, x, loss_mask=m, mask_norm="masked_mean", noise_in=nin, per_sample_loss=True)
    assert not torch.equal(bits(eager["a"][2]), bits(eager["b"][2])) and not torch.equal(bits(eager["a"][2]), bits(g0))

    def same_step(a, b):      # replay against kernel-by-kernel launches: the bar of test_graph_replay_equals_eager_launches
        return abs(a[0][0] - b[0][0]) <= 1e-6 * abs(b[0][0]) and float((a[2] - b[2]).norm() / b[2].norm()) <= 1e-5

    def identical(a, b):
        return a[0] == b[0] and torch.equal(bits(a[1]), bits(b[1])) and torch.equal(bits(a[2]), bits(b[2]))

    step = lambda m: _tiny_step(net, x, loss_mask=m, mask_norm="masked_mean", noise_in=nin, per_sample_loss=True)
    # The same under hipGraph replay, as test_unit_weights_leave_the_gradient_arena_bitwise does it: the loss side (L_b) has the
    # bits of the kernel-by-kernel steps in every call; the gradient arena of a replay is compared bit for bit with another replay
    # of the same mask (the graph orders the two streams' atomics its own way) and with the kernel-by-kernel step at the bar
    # test_graph_replay_equals_eager_launches (test_gpu_model.py) sets for that comparison.
    net.set_graph_mode(True)
    try:
        first = step(ma)                                                       # eager
        captured = step(ma)                                                    # captured
        replay_a = step(ma)                                                    # replayed
        replay_b = step(mb)                                                    # replayed, the mask changed ...
        replay_a2 = step(ma)                                                   # ... and changed back
        replay_b2 = step(mb)
    finally:
        net.set_graph_mode(False)
    for got, want in ((first, eager["a"]), (captured, eager["a"]), (replay_a, eager["a"]), (replay_b, eager["b"]),
                      (replay_a2, eager["a"]), (replay_b2, eager["b"])):
        print(f"[loss-mask] graph step vs kernel-by-kernel: loss {got[0][0]:.8e} / {want[0][0]:.8e}, arena bit-equal "
              f"{torch.equal(bits(got[2]), bits(want[2]))}")
        assert same_step(got, want) and torch.equal(bits(got[1]), bits(want[1]))
    assert identical(replay_a2, replay_a) and identical(replay_b2, replay_b)
    assert not identical(replay_b, replay_a) and not same_step(replay_b, replay_a)
