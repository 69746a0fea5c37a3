"""Per-sample loss weights, per-sample losses and the Huber element losses of the HIP loss kernels (csrc/loss.hip), through the
C ABI `sdxl_op_loss` on the `Case` pattern of test_gpu_loss_goldens.py, then through the whole step on the tiny UNet.

The reference is tests/_loss_ext_ref.py (float64 sums on the SAME bf16-rounded prediction, target and MinSNR weight in fp32 as
the device computes them).  Tolerances are the ones test_gpu_loss_goldens.py uses for the same comparisons: losses 1e-5 relative;
dpred max error <= 2^-8 of the largest reference magnitude and median relative error <= 2^-8 (the bf16 store).

Shapes: B in {1, 4}; 64 x 64 (HW a multiple of the 256-pixel block), 13 x 10 (HW = 130: every block straddles samples, three
of them at most), 104 x 152 at B = 4 (HW = 15 808 = 61.75 blocks: the 832 x 1216 bucket)."""
import ctypes as C

import numpy as np
import pytest
import torch

import sdxl_amd  # noqa: F401
from oracle import loss_ref as R
from oracle import unet_ref as U
from sdxl_amd import lib
from sdxl_amd import unet as NU

import _loss_ext_ref as X
from _gradparity import GradParity, compare_autograd

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
LOSS_RTOL_KERNEL = 1e-5
DPRED_BAR = 2.0 ** -8
SHAPES = [(1, 64, 64), (4, 64, 64), (1, 13, 10), (4, 13, 10), (4, 104, 152)]
METHODS = {"ddpm": 0, "flow_matching": 1}
DDPM_TS = torch.tensor([500, 800, 900, 950])          # sigma 3e2 .. 3e-2: MinSNR both below and at gamma
FLOW_T = torch.tensor([0.2, 0.45, 0.6, 0.85])


@pytest.fixture(scope="module")
def L():
    assert torch.cuda.is_available()
    return lib.load()


def T(a):
    return torch.from_numpy(np.asarray(a))


def _st():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def to_rows8(x_nchw):
    B, Cc, H, W = x_nchw.shape
    o = torch.zeros(B * H * W, 8, dtype=torch.bfloat16, device=DEV)
    o[:, :4] = x_nchw.to(torch.bfloat16).permute(0, 2, 3, 1).reshape(B * H * W, 4).to(DEV)
    return o


def from_rows8(r, B, H, W):
    return r.view(B, H * W, 8)[..., :4].permute(0, 2, 1).reshape(B, 4, H, W).cpu()


def _dev(t):
    return None if t is None else torch.as_tensor(t, dtype=torch.float32).contiguous().to(DEV)


class Case:
    """One call set of sdxl_op_loss on fixed (latents, noise / x0, sigma / t), with the appended fields (a copy of the class in
    test_gpu_loss_goldens.py; `sw` = sample_weights, `hc` = per-sample huber_c, `c` = the scalar, `per_sample` = want L_b)."""

    def __init__(self, L, method, lat, noise, sig, pred_type=1, use_min_snr=1, gamma=5.0, ztsnr=1, tag=None, loss_type=0, c=0.0,
                 sw=None, hc=None, per_sample=False):
        self.L, self.B, self.H, self.W = L, lat.shape[0], lat.shape[2], lat.shape[3]
        self.ps = torch.full((self.B,), -7.0, dtype=torch.float32, device=DEV) if per_sample else None
        self.keep = [_dev(lat), _dev(noise), _dev(sig), _dev(tag), _dev(sw), _dev(hc)]
        ptr = lambda t: None if t is None else t.data_ptr()
        self.lc = lib.LossConfig(method, pred_type, use_min_snr, gamma, ztsnr, loss_type, c)
        self.b = lib.Batch(self.B, self.H, self.W, 77, ptr(self.keep[0]), ptr(self.keep[1]), ptr(self.keep[2]), None, None, None, None,
                           ptr(self.keep[3]), ptr(self.keep[4]), ptr(self.keep[5]), ptr(self.ps))

    def raw(self, pred_nchw, phase, scale=1.0, out=None, dp=None):
        """one sdxl_op_loss call, return code handed back"""
        p8 = to_rows8(pred_nchw)
        return self.L.sdxl_op_loss(C.byref(self.lc), C.byref(self.b), None, C.c_void_p(p8.data_ptr()),
                                   None if dp is None else C.c_void_p(dp.data_ptr()), scale,
                                   None if out is None else C.c_void_p(out.data_ptr()), phase, _st())

    def loss(self, pred_nchw):
        """(out[0..7], L_b or None)"""
        out = torch.zeros(8, dtype=torch.float32, device=DEV)
        lib.check(self.raw(pred_nchw, 1, out=out))
        return out.cpu(), None if self.ps is None else self.ps.cpu()

    def dpred_rows(self, pred_nchw, scale=1.0):
        out = torch.zeros(8, dtype=torch.float32, device=DEV)
        dp = torch.empty(self.B * self.H * self.W, 8, dtype=torch.bfloat16, device=DEV)
        lib.check(self.raw(pred_nchw, 1, out=out))
        lib.check(self.raw(pred_nchw, 2, scale=scale, out=out, dp=dp))
        return dp

    def dpred(self, pred_nchw, scale=1.0):
        return from_rows8(self.dpred_rows(pred_nchw, scale), self.B, self.H, self.W).float()


def bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def make(method, B, H, W, seed):
    """inputs, the fp32 target / MinSNR weight of the device, and a bf16-exact prediction with |pred - target| of order 1"""
    g = torch.Generator().manual_seed(seed)
    lat, noise = torch.randn(B, 4, H, W, generator=g), torch.randn(B, 4, H, W, generator=g)
    sig = R.karras_sigmas()[DDPM_TS[:B]] if method == "ddpm" else FLOW_T[:B].clone()
    target, w = X.target_and_weight(method, lat, noise, sig)
    pred = (target + torch.randn(B, 4, H, W, generator=g)).to(torch.bfloat16).float()
    return lat, noise, sig, target, w, pred


def ref64(pred, target, w, sw=None, loss_type="l2", c=0.0, tag=None, scale=1.0):
    """float64 reference: (loss, L_b, dpred)"""
    p, t, ww = pred.double(), target.double(), w.double()
    s = None if sw is None else torch.as_tensor(sw).double()
    cc = c.double() if torch.is_tensor(c) else c
    tg = None if tag is None else torch.as_tensor(tag).double()
    return (float(X.loss(p, t, ww, s, loss_type, cc, tg)), X.per_sample_loss(p, t, ww, s, loss_type, cc),
            X.dpred(p, t, ww, s, loss_type, cc, tg, scale))


def check_loss(what, got, want, rtol=LOSS_RTOL_KERNEL):
    rel = abs(got - want) / abs(want)
    print(f"[loss-ext] {what}: hip {got:.8e} reference {want:.8e} rel {rel:.2e} (tol {rtol:.0e})")
    assert rel <= rtol, (what, got, want)


def check_per_sample(what, got, want, rtol=LOSS_RTOL_KERNEL):
    rel = ((got.double() - want.double()).abs() / want.double().abs().clamp_min(1e-300))
    print(f"[loss-ext] {what}: L_b hip {[f'{float(v):.6e}' for v in got]} worst rel {float(rel.max()):.2e} (tol {rtol:.0e})")
    assert got.shape == want.shape and float(rel.max()) <= rtol, (what, got, want)


def check_dpred(what, got, want):
    err = (got.double() - want).abs()
    mx, med = float(err.max()) / float(want.abs().max()), float((err / want.abs().clamp_min(1e-30)).median())
    print(f"[loss-ext] {what}: dpred max err / max|ref| {mx:.2e}, median rel {med:.2e} (bar {DPRED_BAR:.2e})")
    assert mx <= DPRED_BAR and med <= DPRED_BAR, (what, mx, med)


# ------------------------------------------------------------------------------------------------ 5. per-sample losses, l2
@pytest.mark.parametrize("B,H,W", SHAPES)
@pytest.mark.parametrize("method", ["ddpm", "flow_matching"])
def test_per_sample_losses_l2(L, method, B, H, W):
    lat, noise, sig, target, w, pred = make(method, B, H, W, seed=100 + B + H)
    cs = Case(L, METHODS[method], lat, noise, sig, per_sample=True)
    out, per = cs.loss(pred)
    loss, want_per, _ = ref64(pred, target, w)
    check_loss(f"{method} {B}x{H}x{W}", float(out[0]), loss)
    check_per_sample(f"{method} {B}x{H}x{W}", per, want_per)
    mean = float(per.double().mean())
    raw = float(out[1]) / pred.numel()
    assert abs(mean - raw) <= LOSS_RTOL_KERNEL * abs(raw), (mean, raw)
    # asking for the per-sample output changes nothing else
    out0, none = Case(L, METHODS[method], lat, noise, sig).loss(pred)
    assert none is None and torch.equal(bits(out0), bits(out))


def test_per_sample_losses_on_the_flow_matching_goldens(L, golden):
    for c in range(int(golden["n_fm_cases"])):
        k = f"fm{c}"
        x0, x1, t, vpred = T(golden[f"{k}_x0"]), T(golden[f"{k}_x1"]), T(golden[f"{k}_t"]), T(golden[f"{k}_vpred"])
        want = T(golden[f"{k}_loss_per_sample"])
        out, per = Case(L, 1, x1, x0, t, per_sample=True).loss(vpred)
        check_per_sample(f"{k} vs the reference's own per-sample losses (fp32 prediction there)", per, want, rtol=1e-3)
        vb = vpred.to(torch.bfloat16).float()
        check_per_sample(k, per, X.per_sample_loss(vb.double(), (x1 - x0).double(), torch.ones(x1.shape[0], dtype=torch.float64)))


# ------------------------------------------------------------------------------------------------ 6. weights
@pytest.mark.parametrize("B,H,W", [(4, 64, 64), (4, 13, 10), (4, 104, 152)])
@pytest.mark.parametrize("method", ["ddpm", "flow_matching"])
def test_unit_and_zero_weights_bitwise(L, method, B, H, W):
    lat, noise, sig, target, w, pred = make(method, B, H, W, seed=200 + H)
    base = Case(L, METHODS[method], lat, noise, sig)
    out0, _ = base.loss(pred)
    dp0 = base.dpred_rows(pred, 0.5)
    ones = Case(L, METHODS[method], lat, noise, sig, sw=torch.ones(B), per_sample=True)
    out1, per1 = ones.loss(pred)
    assert torch.equal(bits(out1), bits(out0))
    assert torch.equal(bits(ones.dpred_rows(pred, 0.5)), bits(dp0))
    sw = torch.tensor([1.0, 0.0, 1.0, 1.0])
    z = Case(L, METHODS[method], lat, noise, sig, sw=sw, per_sample=True)
    _, per = z.loss(pred)
    assert float(per[1]) == 0.0
    assert torch.equal(bits(per[[0, 2, 3]]), bits(per1[[0, 2, 3]]))
    dpz = z.dpred_rows(pred, 0.5).view(B, H * W, 8)
    assert int(bits(dpz[1]).ne(0).sum()) == 0                                   # an all-zero slab, bit for bit
    for b in (0, 2, 3):
        assert torch.equal(bits(dpz[b]), bits(dp0.view(B, H * W, 8)[b])), b
    assert float(dpz[0].float().abs().max()) > 0.0


@pytest.mark.parametrize("B,H,W", SHAPES)
@pytest.mark.parametrize("method", ["ddpm", "flow_matching"])
def test_random_weights(L, method, B, H, W):
    lat, noise, sig, target, w, pred = make(method, B, H, W, seed=300 + B + W)
    g = torch.Generator().manual_seed(5)
    sw = torch.rand(B, generator=g) * 2.0 + 0.05
    tag = torch.rand(B, generator=g) + 0.5
    # alone (MinSNR off) ...
    w1 = torch.ones(B)
    cs = Case(L, METHODS[method], lat, noise, sig, use_min_snr=0, sw=sw, per_sample=True)
    out, per = cs.loss(pred)
    loss, want_per, want_dp = ref64(pred, target, w1, sw, scale=0.25)
    check_loss(f"{method} {B}x{H}x{W} weights alone", float(out[0]), loss)
    check_per_sample(f"{method} {B}x{H}x{W} weights alone", per, want_per)
    check_dpred(f"{method} {B}x{H}x{W} weights alone", cs.dpred(pred, 0.25), want_dp)
    # ... and together with tag_weights and MinSNR
    cs = Case(L, METHODS[method], lat, noise, sig, tag=tag, sw=sw, per_sample=True)
    out, per = cs.loss(pred)
    loss, want_per, want_dp = ref64(pred, target, w, sw, tag=tag, scale=0.25)
    check_loss(f"{method} {B}x{H}x{W} weights + tag + MinSNR", float(out[0]), loss)
    check_per_sample(f"{method} {B}x{H}x{W} weights + tag + MinSNR", per, want_per)
    check_dpred(f"{method} {B}x{H}x{W} weights + tag + MinSNR", cs.dpred(pred, 0.25), want_dp)
    assert float(out[7]) == pytest.approx(float(tag.mean()), rel=1e-6)


# ------------------------------------------------------------------------------------------------ 7. huber / smooth_l1
@pytest.mark.parametrize("B,H,W", SHAPES)
@pytest.mark.parametrize("per_sample_c", [False, True], ids=["scalar_c", "per_sample_c"])
@pytest.mark.parametrize("loss_type", ["huber", "smooth_l1"])
@pytest.mark.parametrize("method", ["ddpm", "flow_matching"])
def test_huber_losses(L, method, loss_type, per_sample_c, B, H, W):
    lat, noise, sig, target, w, pred = make(method, B, H, W, seed=400 + B + H)
    hc = torch.tensor([0.01, 0.1, 1.0, 0.3])[:B] if per_sample_c else None
    c = 0.0 if per_sample_c else 0.1
    sw = torch.tensor([0.5, 2.0, 1.0, 1.5])[:B]
    cs = Case(L, METHODS[method], lat, noise, sig, loss_type=lib.LOSS_TYPES[loss_type], c=c, hc=hc, sw=sw, per_sample=True)
    out, per = cs.loss(pred)
    loss, want_per, want_dp = ref64(pred, target, w, sw, loss_type, hc if per_sample_c else c, scale=0.5)
    what = f"{method} {loss_type} {'c_b' if per_sample_c else 'c'} {B}x{H}x{W}"
    check_loss(what, float(out[0]), loss)
    check_per_sample(what, per, want_per)
    check_dpred(what, cs.dpred(pred, 0.5), want_dp)
    # without weights too (the NULL branch of the Huber kernels)
    cs = Case(L, METHODS[method], lat, noise, sig, loss_type=lib.LOSS_TYPES[loss_type], c=c, hc=hc)
    loss, _, want_dp = ref64(pred, target, w, None, loss_type, hc if per_sample_c else c)
    check_loss(what + " unweighted", float(cs.loss(pred)[0][0]), loss)
    check_dpred(what + " unweighted", cs.dpred(pred), want_dp)


@pytest.mark.parametrize("loss_type,c", [(1, 0.0), (1, -0.5), (2, 0.0), (7, 0.1), (-1, 0.1)])
def test_bad_loss_arguments_launch_nothing(L, loss_type, c):
    lat, noise, sig, target, w, pred = make("ddpm", 4, 13, 10, seed=9)
    cs = Case(L, 0, lat, noise, sig, loss_type=loss_type, c=c, per_sample=True)
    out = torch.full((8,), -3.0, dtype=torch.float32, device=DEV)
    dp = torch.full((4 * 130, 8), -3.0, dtype=torch.bfloat16, device=DEV)
    for phase in (1, 2):
        assert cs.raw(pred, phase, out=out, dp=dp) == 1
        msg = L.sdxl_last_error().decode()
        assert "loss_type" in msg or "huber_c" in msg, msg
    torch.cuda.synchronize()
    assert float(out.min()) == float(out.max()) == -3.0 and float(dp.float().min()) == float(dp.float().max()) == -3.0
    assert float(cs.ps.min()) == float(cs.ps.max()) == -7.0
    with pytest.raises(lib.SdxlError, match="huber_c|loss_type"):
        lib.check(cs.raw(pred, 1, out=out))


# ------------------------------------------------------------------------------------------------ 8. guards
@pytest.mark.parametrize("H,W", [(64, 64), (13, 10)])
@pytest.mark.parametrize("method", ["ddpm", "flow_matching"])
def test_guard_with_per_sample_output(L, method, H, W):
    B = 4
    lat, noise, sig, target, w, pred = make(method, B, H, W, seed=500 + H)
    lat = lat.clone()
    lat[2, 1, H // 2, W // 2] = float("inf")
    cs = Case(L, METHODS[method], lat, noise, sig, per_sample=True)
    out, per = cs.loss(pred)
    assert float(out[0]) == 1000.0 and float(out[7]) == 0.0
    assert not torch.isfinite(per[2]) and bool(torch.isfinite(per[[0, 1, 3]]).all()), per
    _, want_per, _ = ref64(pred, target, w)
    check_per_sample(f"{method} guard 4x{H}x{W}: the finite samples", per[[0, 1, 3]], want_per[[0, 1, 3]])
    assert int(bits(cs.dpred_rows(pred)).ne(0).sum()) == 0


# ------------------------------------------------------------------------------------------------ 9. determinism
@pytest.mark.parametrize("B,H,W", [(4, 13, 10), (4, 104, 152), (4, 64, 64)])
def test_per_sample_losses_are_bitwise_reproducible(L, B, H, W):
    lat, noise, sig, target, w, pred = make("ddpm", B, H, W, seed=600 + H)
    sw = torch.tensor([0.7, 1.3, 2.0, 0.1])
    runs = []
    for _ in range(3):
        cs = Case(L, 0, lat, noise, sig, sw=sw, loss_type=1, c=0.2, per_sample=True)
        out, per = cs.loss(pred)
        runs.append((out, per))
        Case(L, 1, noise, lat, FLOW_T[:B], per_sample=True).loss(pred * 3.0)          # something else through the same scratch
    for out, per in runs[1:]:
        assert torch.equal(bits(per), bits(runs[0][1])) and torch.equal(bits(out), bits(runs[0][0]))


# ------------------------------------------------------------------------------------------------ 10. the whole path, tiny UNet
LOSS_RTOL = 1e-3                       # test_gpu_model.py's bar for the tiny UNet's loss against the fp32 oracle
TINY_GRAD_BAR = (6e-2, 0.995)          # ... and for every gradient tensor: rel-L2, cosine
SW = torch.tensor([1.0, 0.0, 2.0, 1.0])


def tiny_native_cfg(c):
    return NU.make_config(block_out_channels=c.block_out_channels, transformer_layers=c.transformer_layers_per_block,
                          cross_attention_dim=c.cross_attention_dim, addition_time_embed_dim=c.addition_time_embed_dim,
                          pooled_dim=c.pooled_dim)


def make_inputs(cfg, B, H, W, seed):
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g)
    bfr = lambda t: t.to(torch.bfloat16).float()
    return dict(lat=r(B, 4, H, W), noise=r(B, 4, H, W), ehs=bfr(r(B, 77, cfg.cross_attention_dim)),
                pooled=bfr(r(B, cfg.pooled_dim)), tid=torch.tensor([[8.0 * H, 8.0 * W, 0, 0, 8.0 * H, 8.0 * W]] * B))


@pytest.fixture(scope="module")
def tiny():
    cfg = U.tiny_config()
    w = U.synth_weights(cfg, seed=0)
    net = NU.NativeUNet(tiny_native_cfg(cfg))
    net.load_state_dict(w)
    yield cfg, w, net
    net.set_graph_mode(False)
    net.close()


TINY_TS = torch.tensor([610, 230, 820, 450])


def _tiny_step(net, x, **ext):
    sig = R.karras_sigmas()[TINY_TS]
    net.zero_grads()
    net.forward_loss("ddpm", x["lat"].clone(), x["noise"].clone(), sig.clone(), TINY_TS.float(), x["ehs"], x["pooled"], x["tid"], **ext)
    net.backward(1.0, True)
    out = net.read_loss()
    per = net.read_per_sample_loss() if ext.get("per_sample_loss") else None
    torch.cuda.synchronize()
    return out, per, net.grads.clone()


@pytest.mark.parametrize("loss_type", ["l2", "huber"])
def test_weighted_step_every_gradient_matches_oracle(tiny, loss_type):
    cfg, w, net = tiny
    B, H, W = 4, 16, 16
    x = make_inputs(cfg, B, H, W, seed=71)
    c = 0.5
    ext = dict(sample_weights=SW, per_sample_loss=True)
    if loss_type != "l2":
        ext.update(loss_type=loss_type, huber_c=c)
    out, per, _ = _tiny_step(net, x, **ext)
    for t in w.values():
        t.grad = None
        t.requires_grad_(True)
    try:
        sig = R.karras_sigmas()[TINY_TS]
        pred = U.unet_forward(w, R.add_noise(x["lat"], x["noise"], sig), TINY_TS, x["ehs"], x["pooled"], x["tid"], cfg)
        target, mw = X.target_and_weight("ddpm", x["lat"], x["noise"], sig)
        ref = X.loss(pred, target, mw, SW, loss_type, c)
        ref_per = X.per_sample_loss(pred.detach(), target, mw, SW, loss_type, c)
        check_loss(f"tiny {loss_type} weighted", out[0], float(ref.detach()), rtol=LOSS_RTOL)
        assert float(per[1]) == 0.0 and float(ref_per[1]) == 0.0
        check_per_sample(f"tiny {loss_type} weighted", per[[0, 2, 3]], ref_per[[0, 2, 3]], rtol=LOSS_RTOL)
        par = GradParity(f"tiny ddpm {loss_type} weights {SW.tolist()} {B}x{H}x{W}")
        compare_autograd(par, ref, w, lambda k: net.export(k, grad=True))
    finally:
        for t in w.values():
            t.grad = None
            t.requires_grad_(False)
    par.check(TINY_GRAD_BAR, expect=net.param_shapes())


def test_unit_weights_leave_the_gradient_arena_bitwise(tiny):
    cfg, w, net = tiny
    x = make_inputs(cfg, 4, 16, 16, seed=72)
    net.set_graph_mode(False)
    out0, _, g0 = _tiny_step(net, x)
    out1, per1, g1 = _tiny_step(net, x, sample_weights=torch.ones(4), loss_type="l2", per_sample_loss=True)
    assert out0 == out1 and torch.equal(bits(g0), bits(g1))
    assert abs(float(per1.double().mean()) - out1[1] / x["lat"].numel()) <= 1e-5 * out1[1] / x["lat"].numel()
    outw, perw, gw = _tiny_step(net, x, sample_weights=SW, per_sample_loss=True)
    assert not torch.equal(bits(gw), bits(g0)) and float(perw[1]) == 0.0
    assert torch.equal(bits(perw[[0, 3]]), bits(per1[[0, 3]])) and float(perw[2]) == 2.0 * float(per1[2])

    # the same under hipGraph replay: first call eager, second captured, third replayed -- and the replay sees new weights.
    # Replays are compared with each other bit for bit, and with the kernel-by-kernel launches at the bar
    # test_graph_replay_equals_eager_launches (test_gpu_model.py) sets for that comparison.
    def same_step(a, b):
        return abs(a[0][0] - b[0][0]) <= 1e-6 * abs(b[0][0]) and float((a[2] - b[2]).norm() / b[2].norm()) <= 1e-5

    ones = dict(sample_weights=torch.ones(4), per_sample_loss=True)
    net.set_graph_mode(True)
    try:
        base = [_tiny_step(net, x) for _ in range(3)]
        assert all(same_step(b, (out0, None, g0)) for b in base)
        r1 = _tiny_step(net, x, **ones)                                                       # eager
        r2 = _tiny_step(net, x, **ones)                                                       # captured
        for r, b in ((r1, base[0]), (r2, base[1])):
            assert r[0] == b[0] and torch.equal(bits(r[2]), bits(b[2])) and torch.equal(bits(r[1]), bits(per1))
        r3 = _tiny_step(net, x, sample_weights=SW, per_sample_loss=True)                      # replayed, weights changed
        assert same_step(r3, (outw, None, gw)) and torch.equal(bits(r3[1]), bits(perw))
        assert not same_step(r3, base[2])
        r4 = _tiny_step(net, x, **ones)                                                       # ... and changed back
        assert r4[0] == base[2][0] and torch.equal(bits(r4[2]), bits(base[2][2])) and torch.equal(bits(r4[1]), bits(per1))
        # a per-sample c is staged the same way; a scalar c is part of the graph's key
        hub = [_tiny_step(net, x, loss_type="huber", huber_c=torch.tensor([0.5, 0.5, 0.5, 0.5]))[0][0] for _ in range(2)]
        hub.append(_tiny_step(net, x, loss_type="huber", huber_c=torch.tensor([0.5, 0.1, 0.5, 2.0]))[0][0])
        sc = [_tiny_step(net, x, loss_type="huber", huber_c=0.5)[0][0] for _ in range(3)]
        sc2 = [_tiny_step(net, x, loss_type="huber", huber_c=0.1)[0][0] for _ in range(3)]
    finally:
        net.set_graph_mode(False)
    eager_c = _tiny_step(net, x, loss_type="huber", huber_c=torch.tensor([0.5, 0.1, 0.5, 2.0]))[0][0]
    eager_s, eager_s2 = _tiny_step(net, x, loss_type="huber", huber_c=0.5)[0][0], _tiny_step(net, x, loss_type="huber", huber_c=0.1)[0][0]
    near = lambda a, b: abs(a - b) <= 1e-6 * abs(b)
    assert near(hub[0], eager_s) and near(hub[1], eager_s) and near(hub[2], eager_c) and not near(eager_c, eager_s)
    assert all(near(v, eager_s) for v in sc) and all(near(v, eager_s2) for v in sc2) and not near(eager_s, eager_s2)
