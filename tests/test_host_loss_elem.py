"""CPU side of the per-element loss tests (tests/_loss_elem.py): the float64 references stay inside their own bounds when the kernels' formulas are
emulated in fp32 and summed in another order -- at every shape and combination the GPU test runs -- and single defects do not: each mutant fails at a
named output, and for each the figures the aggregate bars (check_dpred 2^-8 / 2^-8, loss 1e-5, L_b 1e-5, the sampler's 1e-5) give are printed."""
import importlib.util
import re
from pathlib import Path

import pytest
import torch

import _loss_elem as E
import _loss_mask_ref as MR
import _sampler_ref as R

ROOT = Path(__file__).resolve().parent.parent


def test_build_flags_carry_no_fast_math():
    """the bounds charge 2^-24 per divide and sqrt: both are correctly rounded only while no fast-math flag reaches hipcc"""
    spec = importlib.util.spec_from_file_location("sdxl_build_flags", ROOT / "sdxl-training-improvements_amd" / "build.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    bad = ("fast", "unsafe", "reciprocal", "approx", "finite-math", "no-signed-zeros", "associative", "daz", "denormals")
    for f in mod.FLAGS:
        assert not any(b in f.lower() for b in bad), f


def test_tree_depths_restate_the_kernels_loops():
    src = (ROOT / "sdxl-training-improvements_amd" / "csrc" / "loss.hip").read_text()
    for loop in ("r += 64", "for (int l = 0; l < 64; ++l)", "sred[0][threadIdx.x] + sred[1][threadIdx.x] + sred[2][threadIdx.x] + sred[3][threadIdx.x]",
                 "sps[0] + sps[1] + sps[2] + sps[3]"):
        assert loop in src, loop
    smp = (ROOT / "sdxl-training-improvements_amd" / "csrc" / "sampler.hip").read_text()
    for loop in ("r += 256", "((sm[0][k] + sm[1][k]) + sm[2][k]) + sm[3][k]"):
        assert loop in smp, loop
    assert E.loss_tree_depth(1) == 78 and E.loss_tree_depth(65) == 79 and E.loss_tree_depth(65, channel_adds=False) == 75
    assert E.sampler_tree_depth(256) == 23 and E.sampler_tree_depth(257) == 24
    # the shapes reach what they are there for
    B, H, W = E.SHAPE_ROWS64
    assert max(hi - lo + 1 for lo, hi in (E.sample_rows(b, H * W) for b in range(B))) > 64
    B, H, W = E.SHAPE_BUCKET
    assert max(hi - lo + 1 for lo, hi in (E.sample_rows(b, H * W) for b in range(B))) <= 64
    assert E.ps_slots(5, 50) == 5 and 255 // 50 + 2 > 5 and E.ps_slots(4, 130) == 3 and E.ps_slots(40, 1) == 40
    assert (E.SAMPLER_SHAPES[-1][1] * E.SAMPLER_SHAPES[-1][2] + 255) // 256 == 257


def test_the_table_reaches_every_branch_at_a_straddling_shape():
    seen = set()
    for name, (B, H, W), method, lt, sw, hc, tag, mask, norm, ps, kind in E.TABLE:
        if (H * W) % 256 == 0:
            continue
        seen |= {("lt", lt), ("method", method), ("sw", sw), ("hc", hc and lt != "l2"), ("c", lt != "l2" and not hc), ("tag", tag), ("mask", mask),
                 ("mm", mask and norm == "masked_mean"), ("ps", ps), ("minsnr", E.table_case(E.TABLE[E.TABLE_IDS.index(name)]).min_snr)}
    want = {("lt", "l2"), ("lt", "huber"), ("lt", "smooth_l1"), ("method", "ddpm"), ("method", "flow_matching")}
    want |= {(k, v) for k in ("sw", "hc", "c", "tag", "mask", "mm", "ps", "minsnr") for v in (True, False)}
    assert want <= seen, want - seen
    assert {t[1] for t in E.TABLE} == {E.SHAPE_STRADDLE, E.SHAPE_ALL5, E.SHAPE_HW1, E.SHAPE_ONE_BLOCK, E.SHAPE_SPILL, E.SHAPE_BUCKET, E.SHAPE_ROWS64}


@pytest.mark.parametrize("name", E.TABLE_IDS)
def test_emulation_stays_inside_every_bound(name):
    cs = E.table_case(E.TABLE[E.TABLE_IDS.index(name)])
    worst = E.check_all(name, cs, E.emulate(cs))
    assert worst <= 1.0


@pytest.mark.parametrize("how", ["clamped", "inf"])
def test_emulation_guard_taken_is_all_zero(how):
    lat, noise, sig, pred = E.graded("flow_matching", *E.SHAPE_STRADDLE, seed=5)
    pred = pred.clone()
    if how == "clamped":
        pred = (pred * 256.0).to(torch.bfloat16).float()       # loss ~ 6e4 > 1000
    else:
        pred[2, 1, 3, 3] = float("inf")
    cs = E.case("flow_matching", lat, noise, sig, pred, per_sample=False, tag=torch.tensor([0.5, 1.0, 1.5, 2.0]))
    r = E.reference(cs)
    assert r.guard and int(r.zero.sum()) == r.zero.numel()
    E.check_all(f"guard {how}", cs, E.emulate(cs), r)


def test_prepare_rows_extends_the_bit_exact_restatement():
    """channels 0..3 are _loss_mask_ref.prepare's bits, from noise_in where given; the cond channels and the zero lanes at Cs 8 and 16"""
    B, H, W = 2, 13, 10
    lat, noise, sig, pred = E.graded("ddpm", B, H, W, seed=7)
    g = torch.Generator().manual_seed(8)
    nin = noise + 0.1 * torch.randn(noise.shape, generator=g)
    for ncond, Cs in ((0, 8), (4, 8), (5, 16), (12, 16)):
        cond = torch.randn(B, ncond, H, W, generator=g) if ncond else None
        for method in ("ddpm", "flow_matching"):
            s = sig if method == "ddpm" else torch.tensor([0.3, 0.8])
            rows = E.prepare_rows(E.case(method, lat, noise, s, pred, noise_in=nin, cond=cond))
            assert tuple(rows.shape) == (B * H * W, Cs)
            want = MR.prepare(method, lat, nin, s).permute(0, 2, 3, 1).reshape(-1, 4)
            assert torch.equal(rows[:, :4].view(torch.int16), want.view(torch.int16))
            assert not torch.equal(rows[:, :4], MR.prepare(method, lat, noise, s).permute(0, 2, 3, 1).reshape(-1, 4))
            assert int(rows[:, 4 + ncond:].view(torch.int16).ne(0).sum()) == 0
            if ncond:
                assert torch.equal(rows[:, 4:4 + ncond], cond.to(torch.bfloat16).permute(0, 2, 3, 1).reshape(-1, ncond))


# ------------------------------------------------------------------------------------------------ single defects
def _ddpm_case(shape=E.SHAPE_STRADDLE, **kw):
    lat, noise, sig, pred = E.graded("ddpm", *shape, seed=305)
    return E.case("ddpm", lat, noise, sig, pred, per_sample=True, **kw)


def _mm_case(shape=E.SHAPE_STRADDLE):
    return _ddpm_case(shape, mask=E.fractional_mask(*shape, seed=11, empty=1), mask_norm="masked_mean", sw=torch.tensor([1.0, 0.5, 2.0, 1.5]))


def _huber_small_d():
    lat, noise, sig, pred = E.graded("ddpm", *E.SHAPE_STRADDLE, seed=306, cancel=True)
    return E.case("ddpm", lat, noise, sig, pred, loss_type="huber", c=0.5, per_sample=True)


def _rows64_case():
    return E.table_case(E.TABLE[E.TABLE_IDS.index("fm-rows64-mean")])


# mutant -> (case builder, victim sample, the output it must fail at, whether the first failing element must lie in the victim)
MUTANT_CASES = {
    "sigma_target": (_ddpm_case, 0, r"d pred:", True),
    "sigma_weight": (_ddpm_case, 0, r"d pred:", True),
    "sigma_both": (_ddpm_case, 0, r"d pred:", True),
    "block_first_sample": (_ddpm_case, 1, r"d pred:", True),      # pixels 130 .. 255 of block 0 read sample 0's sigma
    "hw_for_mb": (_mm_case, 2, r"d pred:", True),
    "mask_late": (_mm_case, 0, r"d pred", False),
    "huber_plain_diff": (_huber_small_d, 0, r"out\[0\]|out\[1\.\.6\]|L_b", False),
    "d_bf16": (_ddpm_case, 0, r"d pred:", False),
    "truncate": (_ddpm_case, 0, r"d pred:", False),
    "pad_lane": (_ddpm_case, 0, r"pad lanes", False),
    "slot_dropped": (_ddpm_case, 3, r"L_b:", True),
    "rows_past_64": (_rows64_case, 1, r"L_b:", True),      # (sample 0 has the empty mask)
}


@pytest.mark.parametrize("mutant", E.MUTANTS)
def test_single_defect_fails_at_its_output(mutant):
    build, victim, where, in_victim = MUTANT_CASES[mutant]
    cs = build()
    r = E.reference(cs)
    E.check_all(f"{mutant}: the unmutated emulation", cs, E.emulate(cs), r)
    got = E.emulate(cs, mutant, victim)
    old = E.old_bars(cs, got, r)
    print(f"[ops-loss] mutant {mutant} {cs.B}x{cs.H}x{cs.W} under the old bars: dpred max/max {old['dpred_max']:.2e} median rel {old['dpred_median']:.2e} "
          f"(bar 3.9e-03: {'passes' if old['passes']['dpred'] else 'fails'}), loss rel {old['loss_rel']:.2e} (1e-5: {'passes' if old['passes']['loss'] else 'fails'}), "
          f"L_b rel {old['lb_rel']:.2e} (1e-5: {'passes' if old['passes']['L_b'] else 'fails'})")
    with pytest.raises(AssertionError, match=where) as ei:
        E.check_all(mutant, cs, got, r)
    msg = str(ei.value)
    print(f"[ops-loss] mutant {mutant} fails here: {msg[:200]}")
    if in_victim:
        i = int(re.search(r"flat index (\d+)", msg).group(1))
        sample = i if "L_b" in msg.split(":")[0] else (i // 4) // cs.HW
        assert sample == victim, (mutant, i, sample)


def test_defects_the_old_bars_let_through():
    """the table of the README: which old bar each mutant passes (asserted, not assumed)"""
    want_pass = {"sigma_target": ("dpred", "loss"), "huber_plain_diff": ("dpred", "loss"), "pad_lane": ("dpred", "loss", "L_b"), "truncate": ("loss", "L_b"),
                 "slot_dropped": ("dpred", "loss"), "rows_past_64": ("dpred", "loss"), "sigma_weight": (), "sigma_both": (), "block_first_sample": (),
                 "hw_for_mb": (), "mask_late": (), "d_bf16": ()}
    assert set(want_pass) == set(E.MUTANTS)
    for mutant, bars in want_pass.items():
        build, victim, _, _ = MUTANT_CASES[mutant]
        cs = build()
        old = E.old_bars(cs, E.emulate(cs, mutant, victim))
        assert {b for b, ok in old["passes"].items() if ok} == set(bars), (mutant, old)


# ------------------------------------------------------------------------------------------------ the sampler's guidance rescale
def _k(phi, cfg=1):
    f = lambda v: float(torch.tensor(v, dtype=torch.float32))
    return dict(cfg=cfg, init=0, a_skip=f(0.3), a_out=f(-0.9), p=f(0.6), q=f(0.4), a_in_next=f(0.5), clamp=0.0, guidance=f(5.0), guidance_rescale=f(phi))


def _check_sampler(tag, got, ref):
    from _nonlinear import check_f32
    return check_f32(tag, got, ref.x, ref.dx)


@pytest.mark.parametrize("ratio", [0.0, 1.0, 8.0])
@pytest.mark.parametrize("B,H,W", E.SAMPLER_SHAPES)
def test_sampler_emulation_stays_inside_its_bound(B, H, W, ratio):
    k = _k(0.7)
    x, fc, fu = E.sampler_data(B, H, W, ratio, seed=40 + H)
    ref = E.sampler_reference(x, fc.float(), fu.float(), k)
    got = E.sampler_emulate(x, fc, fu, k)
    frac = _check_sampler(f"sampler rescale mean/std {ratio:g} {(B, H, W)}", got, ref)
    print(f"[ops-loss] sampler rescale {(B, H, W)} mean/std {ratio:g}: cancellation Q / (Q - S^2/n) F_c {float(ref.cancel_c.max()):.3g} F {float(ref.cancel_f.max()):.3g}, "
          f"ratio bound {float((ref.dratio / ref.ratio).max()):.2e} relative, largest fraction of delta needed {frac:.3g}")
    assert bool(ref.live.all()) and frac <= 1.0


@pytest.mark.parametrize("B,H,W", E.SAMPLER_SHAPES)
def test_sampler_exact_designs_have_the_plain_steps_bits(B, H, W):
    k = _k(0.5)
    for name, (x, fc, fu), kk in (("constant F", E.sampler_constant_f(B, H, W, 50), dict(k, guidance=2.0)), ("+-1", E.sampler_pm1(B, H, W, 51), k)):
        plain, _ = R.full_step(x, fc.float(), fu.float(), dict(kk, guidance_rescale=0.0))
        got = E.sampler_emulate(x, fc, fu, kk)
        assert torch.equal(got.view(torch.int32), plain.view(torch.int32)), name
        if name == "constant F":
            assert float(R.guide(fc.float(), fu.float(), 2.0).std()) == 0.0 and float(fc.float().std()) > 0.5


@pytest.mark.parametrize("mutant,shape", [("rows_past_256", E.SAMPLER_SHAPES[-1]), ("n_for_n1", E.SAMPLER_SHAPES[0])])
def test_sampler_single_defect_fails(mutant, shape):
    B, H, W = shape
    k = _k(0.7)
    x, fc, fu = E.sampler_data(B, H, W, 1.0, seed=60)
    ref = E.sampler_reference(x, fc.float(), fu.float(), k)
    got = E.sampler_emulate(x, fc, fu, k, mutant)
    old = float((got.double() - ref.x).abs().max() / ref.x.abs().max())
    print(f"[ops-loss] sampler mutant {mutant} {shape} under the old bar: max |dx| / max |x_next| {old:.2e} (1e-5: {'passes' if old <= 1e-5 else 'fails'})")
    with pytest.raises(AssertionError, match="x_next"):
        _check_sampler(f"sampler {mutant} x_next", got, ref)
