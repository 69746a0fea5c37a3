"""The CPU restatement of the schedule-free Kahan AdamW (tests/_schedulefree_ref.py) pinned bit-exactly to fixtures produced
by the reference's own `AdamWScheduleFreeKahan` (tests/golden/schedulefree_kahan.npz, tests/make_schedulefree_goldens.py),
and the reason the compensated mode is the default: it tracks an exact-precision restatement of the update, the reference's
literal bf16 arithmetic does not."""
from pathlib import Path

import numpy as np
import pytest

import _schedulefree_ref as S
from oracle.adamw_ref import bf16_to_f32, f32_to_bf16_rn

G = np.load(Path(__file__).parent / "golden" / "schedulefree_kahan.npz")


def hyper(name):
    lr, b1, b2, eps, wd, warm, kahan = (float(x) for x in G[f"{name}_hyper"])
    return lr, b1, b2, eps, wd, int(warm), bool(kahan)


@pytest.mark.parametrize("name", [str(c) for c in G["cases"]])
def test_reference_mode_bit_exact(name):
    lr, b1, b2, eps, wd, warm, kahan = hyper(name)
    p = G[f"{name}_p0"]
    m, v = np.zeros_like(p), np.zeros_like(p)
    c = np.zeros_like(p) if kahan else None
    lr_max = -1.0
    for st in range(1, int(G[f"{name}_steps"]) + 1):
        adjusted_lr, ss = S.schedule(st - 1, lr, b2, warm)
        lr_max = max(lr_max, adjusted_lr)
        assert (adjusted_lr, lr_max) == tuple(G[f"{name}_lr{st}"]), f"{name} step {st}: last_lr / lr_max"
        p, m, v, c, ga = S.step(p, m, v, c, S.grad_in(G[f"{name}_grad{st}"]), step_size=ss, beta1=b1, beta2=b2, eps=eps,
                                weight_decay=wd, kahan_sum=kahan, reference=True)
        got = [("p", p), ("m", m), ("v", v), ("gafter", ga)] + ([("c", c)] if kahan else [])
        for k, a in got:
            want = G[f"{name}_{k}{st}"]
            bad = int((a != want).sum())
            assert bad == 0, f"{name} step {st} {k}: {bad}/{a.size} elements differ (first at {np.flatnonzero(a != want)[:5]})"
        if kahan:
            assert (c == 0).all()                         # defect 1: the reference's compensation is +0 everywhere


def test_warmup_schedule():
    """sched = (k+1)/warmup while k < warmup, adjusted_lr = lr*sched*sqrt(1-beta2^(k+1)), step_size = adjusted_lr/sqrt(...)"""
    got = [S.schedule(k, 1e-3, 0.999, 3) for k in range(5)]
    for k, (a, s) in enumerate(got):
        bc = 1 - 0.999 ** (k + 1)
        assert a == pytest.approx(1e-3 * min(1.0, (k + 1) / 3) * bc ** 0.5, rel=1e-15)
        assert s == pytest.approx(1e-3 * min(1.0, (k + 1) / 3), rel=1e-15)


def _track(reference, steps=20, n=65536, lr=1e-6, wd=0.01):
    """relative distance of the represented parameter (p + c) from a float64 master that applies the same update (the same
    bf16 moments) with decoupled, lr-scaled decay"""
    rng = np.random.default_rng(0)
    p0 = f32_to_bf16_rn((rng.standard_normal(n) * 0.05).astype(np.float32))
    bias = (rng.standard_normal(n) * 1e-3).astype(np.float32)
    gr = np.random.default_rng(1)
    p, m, v, c = p0.copy(), np.zeros_like(p0), np.zeros_like(p0), np.zeros_like(p0)
    x0 = bf16_to_f32(p0).astype(np.float64)
    x = x0.copy()
    for k in range(steps):
        _, ss = S.schedule(k, lr, 0.999, 0)
        g = S.grad_in(bias + (gr.standard_normal(n) * 1e-3).astype(np.float32))
        p, m, v, c, _ = S.step(p, m, v, c, g, step_size=ss, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=wd, kahan_sum=True,
                               reference=reference)
        d = S.rn(S.rn(np.sqrt(bf16_to_f32(v))) + S._bf16_scalar(1e-8)).astype(np.float64)
        x = x - ss * wd * x - ss * (bf16_to_f32(m).astype(np.float64) / d)
    rep = bf16_to_f32(p).astype(np.float64) + bf16_to_f32(c).astype(np.float64)
    return float(np.linalg.norm(rep - x) / np.linalg.norm(x - x0)), float((p != p0).mean())


def test_compensated_tracks_fp32_master():
    err, moved = _track(reference=False)
    print(f"compensated: |(p+c) - x| / |x - x0| = {err:.2e}; {moved:.1%} of the bf16 weights changed")
    assert err <= 1e-2


def test_reference_mode_does_not():
    """defects 2 and 3: at lr 1e-6 the literal bf16 arithmetic rounds the updates away, and its weight decay (not lr-scaled)
    moves the weights by 1 % per step -- far outside the bound the compensated mode keeps"""
    err, _ = _track(reference=True)
    print(f"reference: |p - x| / |x - x0| = {err:.2e}")
    assert err > 1e-2
    err0, _ = _track(reference=True, wd=0.0)             # without decay: the small updates alone are lost
    assert err0 > 1e-2
