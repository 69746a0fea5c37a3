"""The loss kernels (csrc/loss.hip) and the sampler's guidance rescale (csrc/sampler.hip) held per element, through `sdxl_op_loss` and
`sdxl_op_sampler_step`: float64 references from the caller's inputs with derived bounds (tests/_loss_elem.py), exact designs whose sums are the same
bits in any order, every exact zero of the design bit for bit -- the pad lanes of d pred included, the output prefilled with NaN.  tests/_loss_elem.py's
TABLE says which combination runs at which shape; tests/test_host_loss_elem.py shows what these checks see that the aggregate bars do not.
Every case prints the branches it reached and the largest fraction of its bound the kernel needed (profiles/ops_loss.txt)."""
import ctypes as C

import pytest
import torch

import _loss_elem as E
import _sampler_ref as R
import sdxl_amd  # noqa: F401
from sdxl_amd import lib
from _nonlinear import check_bits, check_f32
from test_gpu_loss_ext import DEV, METHODS, _dev, _st
from test_gpu_loss_mask import MaskCase
from test_gpu_sampler import check_image, run_hook

pytestmark = pytest.mark.gpu
BF = torch.bfloat16


@pytest.fixture(scope="module")
def L():
    assert torch.cuda.is_available()
    return lib.load()


def device_case(L, cs):
    return MaskCase(L, METHODS[cs.method], cs.lat, cs.noise, cs.sig, pred_type=cs.prediction_type, use_min_snr=int(cs.min_snr), gamma=cs.gamma,
                    ztsnr=int(cs.ztsnr), tag=cs.tag, loss_type=lib.LOSS_TYPES[cs.loss_type], c=cs.c, sw=cs.sw, hc=cs.hc, per_sample=cs.per_sample,
                    mask=cs.mask, mask_norm=cs.mask_norm, noise_in=cs.noise_in)


def run(L, cs):
    """phases 1 and 2 of sdxl_op_loss; d pred prefilled with NaN: every lane of every row must be written"""
    dc = device_case(L, cs)
    out = torch.full((8,), float("nan"), dtype=torch.float32, device=DEV)
    dp = torch.full((cs.B * cs.HW, 8), float("nan"), dtype=BF, device=DEV)
    lib.check(dc.raw(cs.pred, 1, out=out))
    lib.check(dc.raw(cs.pred, 2, scale=cs.grad_scale, out=out, dp=dp))
    torch.cuda.synchronize()
    return dict(out=out.cpu(), dpred=dp.cpu(), ps=None if dc.ps is None else dc.ps.cpu(), mnorm=None)


@pytest.mark.parametrize("name", E.TABLE_IDS)
def test_loss_kernels_per_element(L, name):
    cs = E.table_case(E.TABLE[E.TABLE_IDS.index(name)])
    worst = E.check_all(name, cs, run(L, cs))
    assert worst <= 1.0


@pytest.mark.parametrize("how", ["clamped", "inf"])
def test_guard_taken_is_an_exact_zero_gradient(L, how):
    lat, noise, sig, pred = E.graded("flow_matching", *E.SHAPE_STRADDLE, seed=5)
    pred = pred.clone()
    if how == "clamped":
        pred = (pred * 256.0).to(BF).float()
    else:
        pred[2, 1, 3, 3] = float("inf")
    cs = E.case("flow_matching", lat, noise, sig, pred, tag=torch.tensor([0.5, 1.0, 1.5, 2.0]))
    r = E.reference(cs)
    assert r.guard
    E.check_all(f"guard {how}", cs, run(L, cs), r)
    # the other branch on the same data: the guard passes the loss through
    cs2 = E.case("flow_matching", lat, noise, sig, E.graded("flow_matching", *E.SHAPE_STRADDLE, seed=5)[3], tag=torch.tensor([0.5, 1.0, 1.5, 2.0]))
    r2 = E.reference(cs2)
    assert not r2.guard
    E.check_all(f"guard not taken ({how})", cs2, run(L, cs2), r2)


def prepare(L, cs):
    """phase 0: the UNet input [B*HW][Cs], prefilled with NaN"""
    dc = device_case(L, cs)
    ncond = 0 if cs.cond is None else cs.cond.shape[1]
    Cs = 8 if 4 + ncond <= 8 else 16
    b = dc.b
    if ncond:
        cond = _dev(cs.cond)
        b = lib.InputCondBatch(*[getattr(dc.b, f[0]) for f in lib.Batch._fields_])
        b.ctx_len |= lib.BATCH_COND
        b.input_cond, b.cond_channels = cond.data_ptr(), ncond
    rows = torch.full((cs.B * cs.HW, Cs), float("nan"), dtype=BF, device=DEV)
    lib.check(L.sdxl_op_loss(C.byref(dc.lc), C.byref(b), C.c_void_p(rows.data_ptr()), None, None, 1.0, None, 0, _st()), "sdxl_op_loss phase 0")
    torch.cuda.synchronize()
    return rows.cpu()


@pytest.mark.parametrize("ncond", [0, 4, 5, 12])
@pytest.mark.parametrize("B,H,W", [E.SHAPE_STRADDLE, E.SHAPE_SPILL])
def test_x_in_is_the_bit_exact_image_of_the_callers_arrays(L, B, H, W, ncond):
    g = torch.Generator().manual_seed(70 + ncond)
    for method in ("ddpm", "flow_matching"):
        lat, noise, sig, pred = E.graded(method, B, H, W, seed=71)
        nin = noise + 0.1 * torch.randn(noise.shape, generator=g)
        cond = torch.randn(B, ncond, H, W, generator=g) if ncond else None
        for noise_in in (None, nin):
            cs = E.case(method, lat, noise, sig, pred, noise_in=noise_in, cond=cond)
            check_bits(f"x_in {method} {(B, H, W)} ncond {ncond} noise_in {noise_in is not None}", prepare(L, cs), E.prepare_rows(cs))
    print(f"[ops-loss] x_in {(B, H, W)} ncond {ncond}: bit-equal, Cs {8 if 4 + ncond <= 8 else 16}, both methods, with and without noise_in")


# ------------------------------------------------------------------------------------------------ the sampler's guidance rescale
def _k(phi, guidance=5.0):
    f = lambda v: float(torch.tensor(v, dtype=torch.float32))
    return dict(cfg=1, init=0, a_skip=f(0.3), a_out=f(-0.9), p=f(0.6), q=f(0.4), a_in_next=f(0.5), clamp=0.0, guidance=f(guidance), guidance_rescale=f(phi))


@pytest.mark.parametrize("ratio", [0.0, 1.0, 8.0])
@pytest.mark.parametrize("B,H,W", E.SAMPLER_SHAPES)
def test_sampler_rescale_per_element(B, H, W, ratio):
    k = _k(0.7)
    x, fc, fu = E.sampler_data(B, H, W, ratio, seed=40 + H)
    ref = E.sampler_reference(x, fc.float(), fu.float(), k)
    assert bool(ref.live.all())
    got_x, xin = run_hook(x, fc, fu, k)
    frac = check_f32(f"sampler rescale x_next mean/std {ratio:g} {(B, H, W)}", got_x, ref.x, ref.dx)
    check_image(xin, R.unet_input(got_x, k["a_in_next"], k["clamp"]), B, H, W, 1)
    print(f"[ops-loss] sampler rescale {(B, H, W)} mean/std {ratio:g}: partial rows {(H * W + 255) // 256}, cancellation Q / (Q - S^2/n) F_c "
          f"{float(ref.cancel_c.max()):.3g} F {float(ref.cancel_f.max()):.3g}, ratio bound {float((ref.dratio / ref.ratio).max()):.2e} relative, largest fraction of "
          f"delta needed {frac:.3g}")
    assert frac <= 1.0


@pytest.mark.parametrize("B,H,W", E.SAMPLER_SHAPES)
def test_sampler_rescale_exact_designs_have_the_plain_steps_bits(B, H, W):
    """constant F: var(F) is an exact zero, not positive, the ratio stays 1; +-1 data: the four sums are integers, the variances equal, the ratio
    exactly 1; with phi = 1/2 the state then has the bits of the step without rescale"""
    for name, (x, fc, fu), k in (("constant F", E.sampler_constant_f(B, H, W, 50), _k(0.5, 2.0)), ("+-1", E.sampler_pm1(B, H, W, 51), _k(0.5))):
        plain, plain_in = R.full_step(x, fc.float(), fu.float(), dict(k, guidance_rescale=0.0))
        got_x, xin = run_hook(x, fc, fu, k)
        check_bits(f"sampler rescale {name} {(B, H, W)} x_next", got_x, plain)
        check_image(xin, plain_in, B, H, W, 1)
    print(f"[ops-loss] sampler rescale {(B, H, W)}: constant F and +-1 designs have the plain step's bits")
